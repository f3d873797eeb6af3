"""Silence, faint stretches and non-finite samples through the kernels that take two signals through one transform, on the GPU and
through the C ABI (inputs, measures and both contracts: tests/dynamics_cases.py; the expectations themselves: tests/test_dynamics_cpu.py).

The library default -- das in double and every fp64 node -- is held to the strict contract per output hop; das in double also gives the
same bytes however the stream is cut into batches.  The fp32 opt-in (BF_DAS_FUSED_F32) is held to the grouped contract.  Every test
asserts with launch_trace that the kernel it is about ran."""
import numpy as np
import pytest

import dynamics_cases as dc
from beamform_amd import capi
from beamform_amd.capi import BF_DAS_F64, BF_DAS_FUSED_F32, BF_INTERLEAVED, BF_PLANAR, launch_trace

pytestmark = pytest.mark.gpu

NAMES = list(dc.MATRIX)
STRETCH = [n for n in NAMES if dc.MATRIX[n]["kind"] == "stretch"]
NAN_ONLY = ["nan_h0", "nan_h8", "nan_h9", "nan_last"]
F = dc.F


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _layout(x, layout):
    """x [M, T] or [S, M, T] planar -> the handle's layout."""
    return np.ascontiguousarray(np.swapaxes(x, -1, -2)) if layout == BF_INTERLEAVED else np.ascontiguousarray(x)


def _cut(xl, layout, a, b, hop):
    return np.ascontiguousarray(xl[..., a * hop:b * hop, :] if layout == BF_INTERLEAVED else xl[..., a * hop:b * hop])


def run_cuts(p, x, cuts, layout=BF_PLANAR, n_streams=1, **kw):
    """The stream x (planar [M, T] or [S, M, T]) through one handle in the batches cuts[i] .. cuts[i + 1] -> (y [S, T] or [T], kernels)."""
    hop = p["hop"]
    bf = capi.Beamformer(p, layout=layout, n_streams=n_streams, **kw)
    xl = _layout(x, layout)
    parts, kernels = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        with launch_trace() as tr:
            parts.append(np.atleast_2d(bf.process(_cut(xl, layout, a, b, hop))))
        kernels += tr.kernels
    bf.close()
    y = np.concatenate(parts, axis=1)
    return (y[0] if n_streams == 1 else y), kernels


def ran(kernels, name):
    assert any(name in k for k in kernels), (name, kernels)


# ---- das in double -------------------------------------------------------------------------------------------------------------------
DAS_F64 = {   # configuration -> microphones, layout, the kernel that must have run
    "planar8": (8, BF_PLANAR, "das_f64_pair_kernel"), "planar4": (4, BF_PLANAR, "das_f64_pair_kernel"), "planar3": (3, BF_PLANAR, "das_f64_pair_kernel"),
    "ring8": (8, BF_INTERLEAVED, "das_f64_ring_kernel"), "ring4": (4, BF_INTERLEAVED, "das_f64_ring_kernel"), "ring2": (2, BF_INTERLEAVED, "das_f64_ring_kernel"),
    "transposed3": (3, BF_INTERLEAVED, "interleaved_to_planar_kernel"), "transposed5": (5, BF_INTERLEAVED, "interleaved_to_planar_kernel"),
    "one_mic": (1, BF_INTERLEAVED, "das_f64_w64_kernel<1>"),
    "chain12": (12, BF_PLANAR, "istft_w64_kernel"),
}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cfg", list(DAS_F64))
def test_das_in_double_meets_the_strict_contract_in_every_batch_plan(cfg, name):
    """Rules 1-3 against the oracle, and rule 4: one batch, the batch cut at (5, 1, rest), a cut at an odd frame inside the stretch (the
    carried hop is loud where the next batch begins with zeros: cut at 7) and, for planar input, one bf_process_hop per callback all
    give the same bytes."""
    M, layout, kernel = DAS_F64[cfg]
    _torch()
    p = dc.params("das", M)
    x = dc.scene(name, M)
    y_ref, _ = dc.ref("das", name, M)
    y, ks = run_cuts(p, x, (0, F), layout, das_impl=BF_DAS_F64)
    ran(ks, kernel)
    if "transposed" in cfg:
        ran(ks, "das_f64_pair_kernel")
    # (one microphone: the hops where the reference is its own rounding noise are held to 1e-12 of the signal's scale instead -- 1e-16 per
    # transform and four orders to spare)
    noise = dc.identity_noise_hops(x, 512) if M == 1 else ()
    dc.check_strict(y, y_ref, 512, f"das in double {cfg} {name}", unpinned=noise, unpinned_abs=1e-12 if M == 1 else None)
    # Rule 4 pins these seeds, it is no guarantee: which frames share a transform depends on the cut, a shared transform leaves 1e-16 of its
    # loudest hop in both frames, and the pairing rule (das_f64_plan.hpp das_f64_may_pair) only bounds how often that flips a last bit of
    # the float output -- 1e-6 per hop on level audio, 3e-5 at most.  Over the 24 hops of a case and all plans a flip is a 1e-3 event; at
    # the parent, and with the rule at 2^20, the transition hops differ in every run.
    for cuts in ((0, 5, 6, F), (0, 7, F), (0, 9, F)):
        y2, _ = run_cuts(p, x, cuts, layout, das_impl=BF_DAS_F64)
        assert np.array_equal(y2, y, equal_nan=True), (cuts, dc.per_hop(y2, y, 512))
    if layout == BF_PLANAR:
        bf = capi.Beamformer(p, das_impl=BF_DAS_F64)
        y3 = np.concatenate([bf.process_hop(x[:, t * 512:(t + 1) * 512]) for t in range(F)])
        bf.close()
        assert np.array_equal(y3, y, equal_nan=True), ("bf_process_hop", dc.per_hop(y3, y, 512))


def _single_batch_digests(cfgs=("planar8", "ring8", "transposed3")):
    """{cfg-name: sha1 of y, its non-finite samples made one NaN}: every case of the matrix in one batch, checked against the oracle on the way."""
    import hashlib
    out = {}
    for cfg in cfgs:
        M, layout, _ = DAS_F64[cfg]
        for name in NAMES:
            y, _ = run_cuts(dc.params("das", M), dc.scene(name, M), (0, F), layout, das_impl=BF_DAS_F64)
            dc.check_strict(y, dc.ref("das", name, M)[0], 512, f"{cfg} {name}")
            # (non-finite samples as one token: a NaN's sign and payload differ between a plain and an atomic add; rule 3 pins where they are)
            out[f"{cfg}-{name}"] = hashlib.sha1(np.where(np.isfinite(y), y, np.float32(np.nan)).view(np.uint32).tobytes()).hexdigest()
    return out


def test_pairs_done_again_at_chunk_boundaries():
    """By default the 24 frames of a case are two chunks, so the pairs the pairing rule does again lie inside a chunk.  With
    BF_DAS_F64_SCHED=1,1 (read once per process: a child) every pair is a chunk of its own: no boundary state on either side, frame tA's
    first half and frame tA + 1's second half go out as atomic adds into zeroed hops -- also in the passes of a pair done again.  Strict
    contract in the child, and the same bytes as the default plan (a chunk plan never changes which frames are paired)."""
    import json
    import os
    import subprocess
    import sys
    _torch()
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_dynamics_gpu as t; "
            "print('RESULT ' + json.dumps(t._single_batch_digests()))" % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BF_DAS_F64_SCHED="1,1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    child = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    mine = _single_batch_digests()
    assert len(child) == 3 * len(NAMES) and child == mine, sorted(k for k in mine if child.get(k) != mine[k])


def test_das_in_double_three_streams_each_with_its_own_trouble():
    _torch()
    names = ("zero_odd", "nan_h9", "m60_even")
    p = dc.params("das", 8)
    x = np.stack([dc.scene(n, 8) for n in names])
    y, ks = run_cuts(p, x, (0, F), n_streams=3, das_impl=BF_DAS_F64)
    ran(ks, "das_f64_pair_kernel")
    for s, n in enumerate(names):
        dc.check_strict(y[s], dc.ref("das", n, 8)[0], 512, f"stream {s} {n}")
    y2, _ = run_cuts(p, x, (0, 5, 6, 9, F), n_streams=3, das_impl=BF_DAS_F64)
    assert np.array_equal(y2, y, equal_nan=True)


@pytest.mark.parametrize("name", NAMES)
def test_das_in_double_tracked_batch_meets_the_strict_contract(name):
    """bf_process_batch_device_tracked, two angles alternating frame by frame: the reference is the oracle with /theta in front of every hop."""
    from track_ref import oracle_tracked
    torch = _torch()
    M, angles = 8, [20.0, -50.0]
    p = dc.params("das", M)
    x = dc.scene(name, M)
    track = np.arange(F, dtype=np.int32) % 2
    y_ref, _ = oracle_tracked(p, x, angles, track, p["theta"])
    bf = capi.Beamformer(p, das_impl=BF_DAS_F64)
    bf.set_track_angles(angles)
    xd, td = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(track).cuda()
    yd = torch.full((F * 512,), float("nan"), dtype=torch.float32, device="cuda")
    with launch_trace() as tr:
        bf.process_device_tracked(xd.data_ptr(), F, yd.data_ptr(), td.data_ptr())
    torch.cuda.synchronize()
    bf.close()
    ran(tr.kernels, "stft_bins_w64_track_kernel")
    ran(tr.kernels, "istft_w64_kernel")
    dc.check_strict(yd.cpu().numpy(), y_ref, 512, f"tracked das in double {name}")


@pytest.mark.parametrize("name", NAMES)
def test_das_in_double_with_the_spectrum_dump_per_frame(name):
    """The dump takes the bin pipeline (stft_bins_w64_kernel: two microphones per transform; istft_w64_kernel): the strict contract on y,
    and rule 2 per frame on Y -- zero frames exactly zero, non-finite frames the oracle's, every other frame within 1e-5 on its own norm."""
    from conftest import rel_l2
    torch = _torch()
    M = 8
    p = dc.params("das", M)
    x = dc.scene(name, M)
    y_ref, Y_ref = dc.ref("das", name, M, want_spectrum=True)
    bf = capi.Beamformer(p, das_impl=BF_DAS_F64)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((F * 512,), float("nan"), dtype=torch.float32, device="cuda")
    Yd = torch.full((F, 1024, 2), float("nan"), dtype=torch.float64, device="cuda")
    with launch_trace() as tr:
        bf.process_device(xd.data_ptr(), F, yd.data_ptr(), Yd.data_ptr())
    torch.cuda.synchronize()
    bf.close()
    ran(tr.kernels, "stft_bins_w64_kernel")
    ran(tr.kernels, "istft_w64_kernel")
    dc.check_strict(yd.cpu().numpy(), y_ref, 512, f"das in double, dump, {name}")
    Y = Yd.cpu().numpy().view(np.complex128)[..., 0]
    fin_ref, fin = np.isfinite(Y_ref).all(axis=1), np.isfinite(Y).all(axis=1)
    assert (fin == fin_ref).all(), (np.flatnonzero(~fin), np.flatnonzero(~fin_ref))
    for t in range(F):
        if not fin_ref[t]:
            continue
        if not Y_ref[t].any():
            assert not Y[t].any(), t
        else:
            assert rel_l2(Y[t], Y_ref[t]) < dc.TOL_TIME, (t, rel_l2(Y[t], Y_ref[t]))


# ---- other periods: the chains of docs/DISPATCH.md -------------------------------------------------------------------------------------
PERIOD_KERNELS = {64: "istft_small_kernel", 256: "istft_small_kernel", 1024: "istft_split_kernel", 2048: "istft_generic_kernel"}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("hop", [64, 256, 1024, 2048])
@pytest.mark.parametrize("algo", ["das", "phase"])
def test_other_periods_meet_the_strict_contract(algo, hop, name):
    """A stretch spans 6 hops at every period (positions in hops, not samples)."""
    _torch()
    M = 8
    p = dc.params(algo, M, hop)
    x = dc.scene(name, M, F, hop)
    y_ref, _ = dc.ref(algo, name, M, F, hop)
    y, ks = run_cuts(p, x, (0, F), das_impl=BF_DAS_F64)
    ran(ks, PERIOD_KERNELS[hop])
    dc.check_strict(y, y_ref, hop, f"{algo} at period {hop} {name}")


# ---- the backward-transform guard, beyond phase --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STRETCH + NAN_ONLY)
@pytest.mark.parametrize("algo,M,interf", [("gss", 8, (-60.0,)), ("mvdr", 4, ())])
def test_backward_transform_guard_under_gss_and_mvdr(algo, M, interf, name):
    """istft_w64_kernel behind gss and mvdr.  mvdr's own NaN frames (frame 0: the inverse of the zero matrix) follow the oracle's
    pattern: rule 3.  (+Inf is left to das and phase: what the reference makes of it in a recursive node hangs on how its FFT library
    orders inf - inf, tests/test_dynamics_cpu.py.)"""
    _torch()
    p = dc.params(algo, M, interf=interf)
    y_ref, _ = dc.ref(algo, name, M, interf=interf)
    y, ks = run_cuts(p, dc.scene(name, M), (0, F))
    ran(ks, "istft_w64_kernel")
    dc.check_strict(y, y_ref, 512, f"{algo} {name}")


def test_phasempf_backward_transform_guard_in_both_paths():
    """mpf_rec_istft_kernel (64 streams) carries a copy of istft_w64_kernel's guard: every case of the matrix on some stream, against
    the oracle under the strict contract and byte for byte against the same stream alone (mpf_recursion_kernel + istft_w64_kernel).
    Where a frame is all zeros phasempf takes arg(+-0 +- 0i) and feeds it to a recursion whose output there is 1e-6 of the signal, not
    zero: oracle/np_oracle.py and the oracle differ by 0.5 to 1.2 on those hops' own norms, so they are left out of rule 2 (the two
    kernels must still agree on them byte for byte)."""
    _torch()
    S, M = 64, 8
    p = dc.params("phasempf", M)
    names = [NAMES[s % len(NAMES)] for s in range(S)]
    xs = np.stack([dc.scene(n, M) for n in names])
    y, ks = run_cuts(p, xs, (0, F), n_streams=S)
    ran(ks, "mpf_rec_istft_kernel")
    assert not any("istft_w64_kernel" in k for k in ks), ks
    for s in range(len(NAMES)):
        y_ref, _ = dc.ref("phasempf", names[s], M)
        dc.check_strict(y[s], y_ref, 512, f"phasempf, 64 streams, stream {s} {names[s]}", unpinned=dc.zero_frame_hops(names[s]))
        one, k1 = run_cuts(p, xs[s], (0, F))
        ran(k1, "mpf_recursion_kernel")
        ran(k1, "istft_w64_kernel")
        assert np.array_equal(one, y[s], equal_nan=True), (names[s], dc.per_hop(one, y[s], 512))


# ---- a dead microphone ---------------------------------------------------------------------------------------------------------------------
DEAD = [(8, 0), (8, 2), (8, 3), (3, 2)]   # index 0, an even index, an odd index, the last of an odd M


@pytest.mark.parametrize("M,dead", DEAD)
@pytest.mark.parametrize("algo,layout", [("das", BF_PLANAR), ("das", BF_INTERLEAVED), ("gsc", BF_PLANAR)])
def test_dead_microphone_under_the_strict_contract(algo, layout, M, dead):
    """das in double and gsc: the reference's answer with an all-zero microphone is well defined."""
    import oracle
    _torch()
    p = dc.params(algo, M)
    x = dc.dead_scene(M, F, 512, dc.SEED + M, dead)
    y_ref, _ = oracle.OracleNode(p).process(x)
    y, ks = run_cuts(p, x, (0, F), layout, das_impl=BF_DAS_F64)
    if algo == "das":
        ran(ks, "das_f64_pair_kernel" if layout == BF_PLANAR or M == 3 else "das_f64_ring_kernel")
    else:
        ran(ks, "gsc_nlms_mw_kernel")
    dc.check_strict(y, y_ref, 512, f"{algo} with microphone {dead} of {M} dead")


def test_mcra_ignores_a_dead_second_microphone():
    """mcra uses channel 0 only (the STFT in front of it takes two microphones through one transform): the output with microphone 1 all
    zeros is the bytes of the run with microphone 1 live."""
    _torch()
    M = 2
    p = dc.params("mcra", M)
    x = dc.stretch_scene(M, F, 512, dc.SEED, 0, 0, 1.0)
    y_live, ks = run_cuts(p, x, (0, F))
    ran(ks, "mcra_node_kernel")
    y_dead, _ = run_cuts(p, dc.dead_scene(M, F, 512, dc.SEED, 1), (0, F))
    assert np.array_equal(y_live, y_dead)
    assert np.isfinite(y_live).all() and y_live.any()


DEAD_NO_PARITY = {"phase": ((), "fused_tail_kernel<8, 4>"), "phasempf": ((), "mpf_recursion_kernel"), "mvdr": ((), "mvdr_fast_kernel"),
                  "lcmv": ((-60.0,), "mvdr_fast_kernel"), "gss": ((-60.0,), "gss_kernel")}


@pytest.mark.parametrize("algo", list(DEAD_NO_PARITY))
def test_dead_microphone_without_a_parity_claim_runs_and_stays_finite(algo):
    """phase / phasempf take arg(+-0 +- 0i) of the dead microphone -- the signs of the reference FFT library's zeros -- and mvdr / lcmv /
    gss a singular covariance: no parity claim (include/bfcore.h).  The node's own kernel runs and the output is finite wherever the
    oracle's is.  For mvdr and lcmv that is nowhere -- the reference inverts the singular covariance into NaN from frame 0 on -- so for
    those two this checks only that the batch runs through the expected kernels and returns."""
    import oracle
    _torch()
    M = 8
    interf, kernel = DEAD_NO_PARITY[algo]
    p = dc.params(algo, M, interf=interf)
    x = dc.dead_scene(M, F, 512, dc.SEED, 2)
    y_ref, _ = oracle.OracleNode(p).process(x)
    y, ks = run_cuts(p, x, (0, F))
    ran(ks, kernel)
    ran(ks, "istft_w64_kernel")
    fin = np.isfinite(y_ref)
    assert fin.any() == (algo not in ("mvdr", "lcmv"))
    assert y.shape == y_ref.shape
    assert np.isfinite(y[fin]).all(), dc.nonfinite_hops(np.where(fin, y, 0.0), 512)


# ---- the fp32 opt-in: the grouped contract ---------------------------------------------------------------------------------------------------
F32 = {   # configuration -> period, microphones, layout, positions in units of k hops, the kernel that must have run
    "regs512": (512, 8, BF_PLANAR, 1, "das_fused_kernel<0, 4, 4, 1>"),
    "group64": (64, 8, BF_PLANAR, 8, "das_fused_kernel<0, 4, 4, 8>"),
    "group128": (128, 8, BF_PLANAR, 4, "das_fused_kernel<0, 4, 4, 4>"),
    "group256": (256, 8, BF_PLANAR, 2, "das_fused_kernel<0, 4, 4, 2>"),
    "il8": (512, 8, BF_INTERLEAVED, 1, "das_fused_il8_kernel"),
    "il4": (512, 4, BF_INTERLEAVED, 1, "das_fused_il_kernel<2, 1>"),
    "wave2048": (1024, 8, BF_PLANAR, 1, "das_fused_wave2048_kernel"),
    "gen4096": (2048, 8, BF_PLANAR, 1, "das_fused_gen_kernel"),
}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cfg", list(F32))
def test_fp32_opt_in_meets_the_grouped_contract(cfg, name):
    """G frames may share a transform (1024 / N below period 512, else 2): errors are bounded at the scale of the loudest hop within
    G + 1, zeros are exact where every input hop within G + 1 is zero, non-finite hops spread by at most G.  Below period 512 the
    positions are scaled by G so that a stretch holds whole groups."""
    hop, M, layout, k, kernel = F32[cfg]
    _torch()
    nF = F * k
    p = dc.params("das", M, hop)
    x = dc.scene(name, M, nF, hop, dc.SEED, k)
    y_ref, _ = dc.ref("das", name, M, nF, hop, dc.SEED, k)
    y, ks = run_cuts(p, x, (0, nF), layout, das_impl=BF_DAS_FUSED_F32)
    ran(ks, kernel)
    dc.check_grouped(y, y_ref, x, hop, f"das fp32 {cfg} {name}")
