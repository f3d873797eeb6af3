"""The cases of the gss post-filter tests (bf_config.gss_postfilter), shared by the CPU check of the inputs
(tests/test_gss_postfilter_cpu.py) and the GPU tests (tests/test_gss_postfilter_gpu.py): the scenes, seeds and rows of
tests/gss_sources_cases.py, filtered by tests/gss_postfilter_ref.py with the case's filter parameters; each computed once per process."""
import functools

import numpy as np

from gss_postfilter_ref import postfilter
from gss_sources_cases import CASES, SEM, case_params, case_ref, sem_params, sem_ref

#: the filter parameters beside phasempf.launch's: the search window short enough to reset inside a test (frame 6), and a milder set
#: that leaves most bins of row 0 above the noise floor (so that an error in Lambda shows, not only one in phase)
LAUNCH5 = dict(mcra_L=5)
MILD = dict(mpf_eta=0.05, mpf_rev_gamma=0.99, mcra_L=5)

#: name -> (case of gss_sources_cases.py, rows R (None: the case's), parameter overrides)
PF_CASES = {
    "g8": ("g8", None, LAUNCH5),
    "g8_mild": ("g8", None, MILD),
    "g4": ("g4", None, {}),                       # S = 1, R = 2: row 1 zero, row 0 filtered with int2 = 0
    "r4s2": ("r4s2", None, LAUNCH5),              # rows 2 and 3 stay exact zeros
    "r1": ("g8", 1, LAUNCH5),                     # R = 1: row 0 alone, int2 = 0
    "l8": ("l8", None, LAUNCH5),                  # lane kernel, 64 streams
    "h64": ("h64", None, LAUNCH5),
    "h256": ("h256", None, LAUNCH5),
    "h2048": ("h2048", None, LAUNCH5),
    "noise": ("small", None, dict(out_only_noise=1, mcra_L=5)),
    "mcra": ("small", None, dict(out_only_mcra=1, mcra_L=5)),
}


def pf_base(name):
    return PF_CASES[name][0]


def pf_rows(name):
    base, R, _ = PF_CASES[name]
    return CASES[base]["R"] if R is None else R


def pf_params(name):
    base, _, over = PF_CASES[name]
    p = case_params(base)
    p.update(over)
    return p


def filtered(p, Y, sources_per_frame):
    """(y [R, F*H] float32, Y' [R, F, N]) of the rows Y: the filter, then gss's backward path with out_amp on every row."""
    from oracle import np_oracle
    Yf = postfilter(p, Y, sources_per_frame)
    y = np.stack([np_oracle.istft_ola(p, Yf[r], p["out_amp"]) for r in range(Yf.shape[0])])
    y.setflags(write=False)
    Yf.setflags(write=False)
    return y, Yf


@functools.lru_cache(maxsize=None)
def pf_ref(name, stream=0, order="blas"):
    """(y [R, F*H] float32, Y [R, F, N] complex128) of one stream of the case, filtered; shared, do not modify."""
    base = pf_base(name)
    _, Y = case_ref(base, stream, order)
    return filtered(pf_params(name), Y[:pf_rows(name)], len(CASES[base]["interf"]) + 1)


# ---- stream semantics: the SEM case of gss_sources_cases.py; the third source exists from the fourth piece on ----------------------------
def sem_pf_params(theta=None):
    p = sem_params(theta)
    p.update(LAUNCH5)
    return p


def sem_sources_per_frame():
    cuts = SEM["cuts"]
    S0 = len(SEM["interf"]) + 1
    return np.array([S0 if t < cuts[3] else S0 + 1 for t in range(SEM["F"])])


@functools.lru_cache(maxsize=None)
def sem_pf_ref(theta0=None, retarget=True, order="blas"):
    _, Y = sem_ref(theta0, retarget, order)
    return filtered(sem_pf_params(theta0), Y, sem_sources_per_frame())


# ---- a scene with a silent tail: behind a closed gate the rows r >= 1 are exact zeros, which the filter turns into noise_floor -----------
SILENT = dict(M=8, interf=(-60.0, 90.0), R=3, F=20, seed=9900)


def silent_params():
    from beamform_amd.params import make_params
    return make_params("gss", n_mics=SILENT["M"], theta=20.0, interf=SILENT["interf"], **LAUNCH5)


@functools.lru_cache(maxsize=None)
def silent_scene():
    from beamform_amd.synth import make_scene
    return make_scene(SILENT["M"], SILENT["F"], seed=SILENT["seed"])     # silent_frac = 0.1: the last two frames


@functools.lru_cache(maxsize=None)
def silent_rows(order="blas"):
    import oracle
    from gss_sources_ref import gss_sources
    p = silent_params()
    _, Y = gss_sources(p, silent_scene(), [(SILENT["F"], oracle.OracleNode(p).weights())], SILENT["R"], order)
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def silent_ref(order="blas"):
    return filtered(silent_params(), silent_rows(order), len(SILENT["interf"]) + 1)
