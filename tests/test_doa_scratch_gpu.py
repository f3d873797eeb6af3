"""bf_doa's scratch across methods on one handle: the three methods share the chunk buffers (spectra, hop flags, partial sums, work
space), which grow to the largest launch plan so far.  A handle that went through other methods and batch sizes gives the bytes of a
fresh handle of the method."""
import numpy as np
import pytest

from beamform_amd.params import AIRA16_XY, make_params
from beamform_amd.synth import make_scene

pytestmark = pytest.mark.gpu

SR = 48000.0
# 9 microphones: an odd count above 8, so Capon and MUSIC take the work-space path and SRP-PHAT the kernel with a run-time count
M, HOP, W = 9, 128, 4
ANGLES = np.linspace(-180.0, 180.0, 8, endpoint=False)
STEPS = [  # method, frames, eig; what grows on the shared handle
    ("srp_phat", 16, False),   # the first allocation
    ("music", 64, True),       # spectra, partial sums (the eigenvalue rows behind the angle rows) and the work space
    ("srp_phat", 128, False),  # hop flags (and spectra, partial sums)
    ("capon", 32, False),      # nothing
]


def _doa(method):
    from beamform_amd.capi import Doa
    doa = Doa(make_params("das", n_mics=M, hop=HOP, mics=AIRA16_XY[:M]), ANGLES, 100.0, 16000.0, W)
    doa.set_method(method)
    if method == "music":
        doa.set_sources(2)
    return doa


def test_scratch_growth_across_methods_keeps_the_bytes():
    x = make_scene(M, 128, HOP, SR, seed=31, mics=AIRA16_XY[:M])
    shared = _doa("srp_phat")
    for step, (method, F, eig) in enumerate(STEPS):
        xs = np.ascontiguousarray(x[:, :F * HOP])
        shared.reset()
        shared.set_method(method)
        if method == "music":
            shared.set_sources(2)
        got = shared.process(xs, eig=eig)
        fresh = _doa(method)
        want = fresh.process(xs, eig=eig)
        fresh.close()
        assert len(got) == len(want) == (3 if eig else 2)
        for name, g, w in zip(("map", "peak", "eig"), got, want):
            assert g.shape == w.shape and g.dtype == w.dtype, (step, method, name)
            assert g.tobytes() == w.tobytes(), (step, method, name)
        assert np.all(np.isfinite(got[0])) and got[0].shape == (F // W, len(ANGLES)), (step, method)
    shared.close()
