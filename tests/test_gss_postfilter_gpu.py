"""gss's multi-source post-filter (bf_config.gss_postfilter = 1; gss_postfilter_kernel): the filtered rows of each beam through the C
ABI against the numpy reference tests/gss_postfilter_ref.py (tied to the phasempf oracle and bounded in its sensitivity to the
rounding of its inputs by tests/test_gss_postfilter_cpu.py).  Every row is judged on its own at the suite's 1e-5 per-frame relative
L2, on the spectrum dump and on the time signal; what the definition makes zero (out of band, bin 0, rows >= S) must be exactly
zero.  Output buffers start as NaN."""
import numpy as np
import pytest

from beamform_amd.capi import BfError, launch_trace
from beamform_amd.synth import make_scene
from gss_postfilter_cases import (LAUNCH5, PF_CASES, SILENT, pf_base, pf_params, pf_ref, pf_rows, sem_pf_params, sem_pf_ref, silent_params,
                                  silent_ref, silent_rows, silent_scene)
from gss_sources_cases import CASES, SEEDS, SEM, case_scene, case_streams, sem_scene
from test_gss_sources_gpu import _bf, _sem_controls, _sem_pieces, _torch, check_rows, check_time, inband, run_dev

pytestmark = pytest.mark.gpu


def check_filtered(p, y, Y, y_ref, Y_ref, S):
    check_rows(p, y, Y, y_ref, Y_ref)
    assert not Y[:, :, 0].any(), "output bin 0 is zero"
    assert not Y[S:].any() and not y[S:].any(), "rows beyond the source count stay exact zeros"


def _one_stream_case(name, **kw):
    base, p, R = pf_base(name), pf_params(name), pf_rows(name)
    F = CASES[base]["F"]
    bf = _bf(p, gss_out_sources=R, gss_postfilter=1, **kw)
    with launch_trace() as tr:
        y, Y = run_dev(bf, case_scene(base), F)
    bf.close()
    S = len(CASES[base]["interf"]) + 1
    y_ref, Y_ref = pf_ref(name)
    assert Y.shape == (R, F, 2 * p["hop"])
    check_filtered(p, y, Y, y_ref, Y_ref, S)
    return tr.kernels


@pytest.mark.parametrize("name", ["g8", "g8_mild", "g4"])
def test_group_kernel_rows_filtered(name):
    """Behind gss_kernel_all at hop 512: the launch values and the milder set (an error in Lambda shows on the bins above the floor),
    both with a search window that resets inside the batch; g4: one source, two rows -- row 0 filtered with int2 = 0, row 1 zero."""
    kernels = _one_stream_case(name)
    assert any("gss_kernel_all<" in k for k in kernels) and not any("gss_lane" in k for k in kernels), kernels


def test_more_rows_than_sources():
    """R = 4 over two sources: rows 2 and 3 stay exact zeros in the spectrum and in time (check_filtered)."""
    _one_stream_case("r4s2")


def test_one_row():
    """R = 1: the reference node's single output, filtered with int2 = 0, behind the very kernel it always ran."""
    kernels = _one_stream_case("r1")
    assert not any("_all<" in k for k in kernels), kernels


@pytest.mark.parametrize("name", ["noise", "mcra"])
def test_out_only_noise_and_out_only_mcra(name):
    _one_stream_case(name)


@pytest.mark.parametrize("name", ["h64", "h256", "h2048"])
def test_other_fft_sizes(name):
    _one_stream_case(name)


def test_trace_names_the_kernel_exactly_when_the_field_is_set():
    """... between the gss kernel and the spectrum dump; and with the field 0 the output equals, byte for byte, that of a handle
    created without setting it."""
    c, p = CASES["g8"], pf_params("g8")
    out = {}
    for key, kw in (("unset", {}), ("off", dict(gss_postfilter=0)), ("on", dict(gss_postfilter=1))):
        bf = _bf(p, gss_out_sources=c["R"], **kw)
        with launch_trace() as tr:
            y, Y = run_dev(bf, case_scene("g8"), c["F"])
        bf.close()
        out[key] = (y, Y, tr.kernels)
    for key in ("unset", "off"):
        assert not any("gss_postfilter_kernel" in k for k in out[key][2]), out[key][2]
    k_on = out["on"][2]
    hits = [i for i, k in enumerate(k_on) if "gss_postfilter_kernel" in k]
    assert len(hits) == 1, k_on
    i_gss = next(i for i, k in enumerate(k_on) if "gss_kernel" in k)
    i_exp = next(i for i, k in enumerate(k_on) if "expand_spectrum_kernel" in k)
    assert i_gss < hits[0] < i_exp, k_on
    assert [k for k in k_on if "gss_postfilter_kernel" not in k] == out["off"][2]
    assert out["off"][0].tobytes() == out["unset"][0].tobytes() and out["off"][1].tobytes() == out["unset"][1].tobytes()
    assert not np.array_equal(out["on"][1], out["off"][1])


def test_lane_kernel_rows_filtered():
    """Behind gss_lane_kernel_all: 64 streams, two uneven batches (the filter's state carries), streams 0, 1, 31 and 63 against the
    reference, every row."""
    name = "l8"
    c, p = CASES[name], pf_params(name)
    n, F, H, R = c["streams"], c["F"], p["hop"], c["R"]
    keep = case_streams(name)
    xs = np.stack([case_scene(name, s) if s in keep else make_scene(c["M"], F, hop=H, seed=SEEDS[name] + 1000 * s, silent_frac=0.0)
                   for s in range(n)])
    bf = _bf(p, n_streams=n, gss_out_sources=R, gss_postfilter=1)
    ys, Ys = [], []
    for a, b in ((0, 3), (3, F)):
        with launch_trace() as tr:
            y, Y = run_dev(bf, xs[:, :, a * H:b * H], b - a)
        assert any("gss_lane_kernel" in k for k in tr.kernels) and any("gss_postfilter_kernel" in k for k in tr.kernels), tr.kernels
        ys.append(y)
        Ys.append(Y)
    bf.close()
    y, Y = np.concatenate(ys, axis=1), np.concatenate(Ys, axis=1)
    assert np.isfinite(y).all() and np.isfinite(Y).all()
    for s in keep:
        y_ref, Y_ref = pf_ref(name, s)
        check_filtered(p, y[s * R:(s + 1) * R], Y[s * R:(s + 1) * R], y_ref, Y_ref, 3)


def _sem_run(**kw):
    bf = _bf(sem_pf_params(), gss_out_sources=SEM["R"], gss_postfilter=1, **kw)
    return bf


def test_stream_semantics_across_batches():
    """/theta in front of the third piece, a third source in front of the fourth: row 2 is zero and its state cold until it exists;
    rows 0 and 1 keep their noise state through both control calls (the reference never restarts it)."""
    bf = _sem_run()
    ys, Ys = [], []
    for i, (n, x) in enumerate(_sem_pieces()):
        _sem_controls(bf, i)
        y, Y = run_dev(bf, x, n)
        ys.append(y)
        Ys.append(Y)
    bf.close()
    y, Y = np.concatenate(ys, axis=1), np.concatenate(Ys, axis=1)
    y_ref, Y_ref = sem_pf_ref()
    p = sem_pf_params()
    check_rows(p, y, Y, y_ref, Y_ref)
    t3 = SEM["cuts"][3]
    assert not Y[:, :, 0].any()
    assert not Y[2, :t3].any() and Y[2, t3:].any() and not y[2, :t3 * 512].any()


def test_two_look_directions_have_their_own_rows_and_state():
    """n_dirs = 2: bf_set_theta moves direction 0 only, so the two beams separate -- and are filtered -- differently."""
    bf = _sem_run(n_dirs=2)
    ys = []
    for i, (n, x) in enumerate(_sem_pieces()):
        _sem_controls(bf, i)
        y = bf.process(x)
        assert y.shape == (2, SEM["R"], n * 512)
        ys.append(y)
    bf.close()
    y = np.concatenate(ys, axis=2)
    check_time(y[0], sem_pf_ref(None, True)[0])
    check_time(y[1], sem_pf_ref(None, False)[0])
    assert not np.array_equal(y[0], y[1])


def test_cut_invariance_bit_for_bit():
    """One batch of 36 frames, the pieces (5, 1, 11, 19) -- a cut at frame 6, where current_L resets with mcra_L = 5 -- and 36
    bf_process_hop calls: the recursion is serial per lane, so the bytes are the same."""
    p, x, F = sem_pf_params(), sem_scene(), SEM["F"]
    bf = _sem_run()
    y1, Y1 = run_dev(bf, x, F)
    bf.close()
    bf = _sem_run()
    ys, Ys, t = [], [], 0
    for n in (5, 1, 11, 19):
        y, Y = run_dev(bf, np.ascontiguousarray(x[:, t * 512:(t + n) * 512]), n)
        ys.append(y)
        Ys.append(Y)
        t += n
    bf.close()
    assert t == F
    assert np.array_equal(np.concatenate(Ys, axis=1), Y1)
    assert np.array_equal(np.concatenate(ys, axis=1), y1)
    bf = _sem_run()
    out = [bf.process_hop(x[:, t * 512:(t + 1) * 512]) for t in range(F)]
    bf.close()
    assert np.array_equal(np.concatenate(out, axis=1), y1)
    assert np.isfinite(y1).all() and Y1[:2, :, inband(p)].all(axis=2).any()


def test_silent_tail():
    """Behind a closed gate the rows r >= 1 are exact zeros: once Lambda > 0 the filter turns an in-band zero into (noise_floor, 0);
    out of band everything stays 0 -- as the reference has it."""
    p, F, R = silent_params(), SILENT["F"], SILENT["R"]
    bf = _bf(p, gss_out_sources=R, gss_postfilter=1)
    y, Y = run_dev(bf, silent_scene(), F)
    bf.close()
    y_ref, Y_ref = silent_ref()
    check_filtered(p, y, Y, y_ref, Y_ref, 3)
    Y_in = silent_rows()
    band = inband(p)
    band[0] = False
    zero_in = (Y_in[1:, F - 1] == 0) & band[None]          # rows 1 and 2 of the last frame: exact-zero inputs in band
    assert zero_in.mean() > 0.3, zero_in.mean()
    assert (Y_ref[1:, F - 1][zero_in] == p["noise_floor"]).all()
    assert (Y[1:, F - 1][zero_in] == p["noise_floor"]).all()
    assert not Y[:, :, ~inband(p)].any()


def test_checkpoint_reset_and_blob_header():
    from beamform_amd.params import make_params
    _torch()
    M, F, R = 4, 16, 3
    p = make_params("gss", n_mics=M, theta=10.0, interf=(-60.0,), **LAUNCH5)
    x = make_scene(M, 2 * F, seed=2)
    first, second = np.ascontiguousarray(x[:, : F * 512]), np.ascontiguousarray(x[:, F * 512:])
    a = _bf(p, gss_out_sources=R, gss_postfilter=1)
    fresh = a.get_state()
    a.process(first)
    blob = a.get_state()
    ya2 = a.process(second)
    b = _bf(p, gss_out_sources=R, gss_postfilter=1)
    b.process(np.ascontiguousarray(x[:, : 3 * 512]))  # scramble b's state first
    b.set_state(blob)
    yb2 = b.process(second)
    assert ya2.shape == (R, F * 512) and np.isfinite(ya2).all() and ya2.tobytes() == yb2.tobytes()
    off = _bf(p, gss_out_sources=R)
    off.process(first)
    blob_off = off.get_state()
    N, So = 1024, 1
    assert len(blob) == len(blob_off) + So * R * (7 * N + 8) * 8
    with pytest.raises(BfError):
        a.set_state(blob_off)
    with pytest.raises(BfError):
        a.set_state(blob_off + bytes(len(blob) - len(blob_off)))      # long enough: the header tells the two apart
    with pytest.raises(BfError):
        off.set_state(blob)
    off.set_state(blob_off)
    a.reset()
    assert a.get_state() == fresh
    ya = a.process(first)
    c = _bf(p, gss_out_sources=R, gss_postfilter=1)
    assert c.process(first).tobytes() == ya.tobytes()
    for h in (a, b, off, c):
        h.close()
