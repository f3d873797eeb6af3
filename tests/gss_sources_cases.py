"""The shapes of the all-sources gss tests, shared by the CPU check of the reference (tests/test_gss_sources_cpu.py) and the GPU
tests (tests/test_gss_sources_gpu.py): name -> scene, parameters and the reference's rows, each computed once per process.

Scenes have no silent tail (silent_frac = 0): behind a closed gate the rows r >= 1 are exact zeros (gss.cpp:139-141), and the CPU
check asks every row r < S for a norm within 1e-6 of row 0's in every frame, so that the per-row tolerance is not spent on a row of
rounding noise.  Gates still close bin by bin (the scene's per-bin magnitude sits around the launch file's threshold)."""
import functools

import numpy as np

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene
from gss_sources_ref import circle_mics, gss_sources

#: name -> M, interferers, R, F, hop, seed, and for the lane-kernel cases the stream count and the streams compared
CASES = {
    # group kernel, hop 512, one stream
    "g8": dict(M=8, interf=(-60.0, 90.0), R=3, F=24),
    "g4": dict(M=4, interf=(), R=2, F=16),                       # S = 1: row 1 exactly zero
    "g16": dict(M=16, interf=(-60.0, 90.0, 150.0), R=4, F=12),
    "g20": dict(M=20, interf=(90.0,), R=2, F=8),                 # above 16 microphones: the sums walk LDS instead of DPP butterflies
    # more rows than sources
    "r4s2": dict(M=8, interf=(-60.0,), R=4, F=8),
    # lane kernel: 64 streams at hop 512, 176 at hop 128 (two wavefronts per CU on 256 CUs)
    "l8": dict(M=8, interf=(-60.0, 90.0), R=3, F=10, streams=64),
    "l7": dict(M=7, interf=(-60.0,), R=2, F=10, streams=64),
    "l6": dict(M=6, interf=(-60.0, 90.0, 150.0), R=4, F=8, hop=128, streams=176),
    # the other FFT sizes
    "h64": dict(M=4, interf=(-60.0,), R=2, F=10, hop=64),
    "h256": dict(M=4, interf=(-60.0,), R=2, F=9, hop=256),
    "h1024": dict(M=4, interf=(-60.0,), R=2, F=8, hop=1024),
    "h2048": dict(M=4, interf=(-60.0,), R=2, F=7, hop=2048),
    "h4096": dict(M=4, interf=(-60.0,), R=2, F=6, hop=4096),
    # layout / precision / rms
    "small": dict(M=8, interf=(-60.0, 90.0), R=3, F=8),
}
SEEDS = {name: 9100 + 17 * i for i, name in enumerate(CASES)}
LANE_STREAMS = lambda n: (0, 1, 31, n - 1)   # noqa: E731  the streams of a lane-kernel batch that are compared


def case_params(name):
    c = CASES[name]
    over = {"mics": circle_mics(c["M"])} if c["M"] > 16 else {}
    return make_params("gss", n_mics=c["M"], hop=c.get("hop", 512), theta=20.0, interf=c["interf"], **over)


@functools.lru_cache(maxsize=None)
def case_scene(name, stream=0):
    c, p = CASES[name], case_params(name)
    return make_scene(c["M"], c["F"], hop=p["hop"], seed=SEEDS[name] + 1000 * stream, mics=p["mics"], silent_frac=0.0)


def case_streams(name):
    n = CASES[name].get("streams", 1)
    return LANE_STREAMS(n) if n > 1 else (0,)


@functools.lru_cache(maxsize=None)
def case_ref(name, stream=0, order="blas"):
    """(y [R, F*H] float32, Y [R, F, N] complex128) of one stream of the case; shared, do not modify."""
    import oracle
    c, p = CASES[name], case_params(name)
    C = oracle.OracleNode(p).weights()
    y, Y = gss_sources(p, case_scene(name, stream), [(c["F"], C)], c["R"], order)
    y.setflags(write=False)
    Y.setflags(write=False)
    return y, Y


# ---- stream semantics: /theta and a structural interferer change between batches ---------------------------------------------------------
SEM = dict(M=8, interf=(-60.0,), R=3, F=36, cuts=(0, 5, 6, 17, 36), theta0=20.0, theta1=-40.0, new_interf=90.0, seed=9700)


def sem_params(theta=None):
    return make_params("gss", n_mics=SEM["M"], theta=SEM["theta0"] if theta is None else theta, interf=SEM["interf"])


@functools.lru_cache(maxsize=None)
def sem_scene():
    return make_scene(SEM["M"], SEM["F"], seed=SEM["seed"], silent_frac=0.0)


def sem_segments(theta0=None, retarget=True):
    """The segments of the stream for one look direction: cold start, a batch cut, /theta in front of the third piece (only where
    `retarget`: bf_set_theta moves look direction 0), a second interferer in front of the fourth (quirk Q3 included: the constraint
    matrices come from the oracle's own control calls)."""
    import oracle
    node = oracle.OracleNode(sem_params(theta0))
    cuts = SEM["cuts"]
    n = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    segs = [(n[0], node.weights()), (n[1], None)]
    if retarget:
        node.set_theta(SEM["theta1"])
        segs.append((n[2], node.weights()))
    else:
        segs.append((n[2], None))
    node.set_interference(2, SEM["new_interf"])
    segs.append((n[3], node.weights()))
    return segs


@functools.lru_cache(maxsize=None)
def sem_ref(theta0=None, retarget=True, order="blas"):
    y, Y = gss_sources(sem_params(theta0), sem_scene(), sem_segments(theta0, retarget), SEM["R"], order)
    y.setflags(write=False)
    Y.setflags(write=False)
    return y, Y
