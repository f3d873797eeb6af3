"""The gsc cases shared by tests/test_gsc_cpu.py (are the cases worth running?) and tests/test_gsc_gpu.py (parity on the device).

A case is (name, M, hop, F, layout, streams, overrides, env, kernels): `overrides` are make_params fields, `env` the environment of the
process that runs it (switches are read once per process: a case with an `env` runs in a child), `kernels` what one batch of it must
launch, written down here from docs/DISPATCH.md and the rule in chain_plan.hpp's comments and NOT computed by the code under test:
test_gsc_cpu.py holds chain_decide to it, test_gsc_gpu.py the launch trace.  Every case stays at or below 8192 samples per stream.

The figures behind each case are measured on the oracle alone by test_gsc_cpu.py (`python tests/test_gsc_cpu.py` prints them):
  d    relative L2 distance between the oracle's output and the upper beamformer alone (how much the cancelling path does; the parity
       bar is 1e-5, so d >= 1e-3 makes idle or wrongly updated filters a failure by two orders of magnitude)
  b2   share of (sample, branch) steps that take the second step-size branch, mu0 / branch power (gsc.cpp:153-157)
  nf   share of them whose step size came out non-finite and was zeroed
  open share of samples with the adaptation gate open (gsc.cpp:147)
  tap  the largest filter coefficient at the end
  o2o  relative L2 distance between the two restatements of the oracle (C++ and numpy; different FFTs)
"""
from collections import namedtuple

import numpy as np

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene

PLANAR, INTERLEAVED = 0, 1       # bf_layout
SERIAL = {"BF_GSC_SERIAL": "1"}

Case = namedtuple("Case", "name M hop F layout streams over env kernels seed zero")


def chain(hop, layout, nlms):
    """docs/DISPATCH.md's gsc rows: the forward transform, the alignment, the backward transform of the period, then the NLMS kernel."""
    n = 2 * hop
    front, back = {128: ("stft_small_kernel<%d, false>", ["istft_small_kernel"]),
                   256: ("stft_small_kernel<%d, false>", ["istft_small_kernel"]),
                   512: ("stft_small_kernel<%d, false>", ["istft_small_kernel"]),
                   1024: ("stft_kernel<%d, false>", ["istft_w64_kernel<false>"]),
                   2048: ("stft_wave2048_kernel<%d, false>", ["istft_split_kernel"]),
                   4096: ("stft_generic_kernel<%d>", ["istft_generic_kernel", "ola_generic_kernel"]),
                   8192: ("stft_generic_kernel<%d>", ["istft_generic_kernel", "ola_generic_kernel"])}[n]
    return [f"n{n}::{k}" for k in [front % layout, "gsc_align_kernel"] + back + [nlms]]


CASES = []


def _add(name, M, hop, F, fs, kernel, layout=PLANAR, streams=1, env=None, zero=None, input_of=None, **over):
    """kernel: the NLMS instantiation -- gsc_nlms_par_kernel<NBM, KPL> (one blocking branch), gsc_nlms_mw_kernel<NW, NBL, KPL> (NW wavefronts,
    NBL branches each) or, BF_GSC_SERIAL=1, gsc_nlms_kernel<NBM, KPL>; KPL = 64-tap groups per lane.  input_of: the case whose scene
    this one shares."""
    assert name not in [c.name for c in CASES] and F * hop <= 8192
    seed = 4000 + len(CASES) if input_of is None else [c.seed for c in CASES if c.name == input_of][0]
    CASES.append(Case(name, M, hop, F, layout, streams, dict(gsc_filter_size=fs, **over), dict(env or {}), chain(hop, layout, kernel), seed, zero))


# ---- filter sizes at hop 512: below, at and above every 64-tap group; 1 and 2: the output window without its newest element is empty / one tap
_add("fs1-m4", 4, 512, 8, 1, "gsc_nlms_mw_kernel<4, 1, 1>")  # d 2.0e-03 b2 0.00 nf 0.00 open 1.00 tap 9.3e-04 o2o 0e+00
_add("fs2-m4", 4, 512, 8, 2, "gsc_nlms_mw_kernel<4, 1, 1>")  # d 3.3e-03 b2 0.00 nf 0.00 open 1.00 tap 2.2e-03 o2o 0e+00
_add("fs63-m4", 4, 512, 8, 63, "gsc_nlms_mw_kernel<4, 1, 1>")  # d 3.3e-02 b2 0.00 nf 0.00 open 1.00 tap 8.9e-03 o2o 0e+00
_add("fs64-m4", 4, 512, 8, 64, "gsc_nlms_mw_kernel<4, 1, 1>")  # d 3.5e-02 b2 0.00 nf 0.00 open 1.00 tap 1.0e-02 o2o 0e+00
_add("fs65-m4", 4, 512, 8, 65, "gsc_nlms_mw_kernel<4, 1, 2>")  # d 2.8e-02 b2 0.00 nf 0.00 open 1.00 tap 7.3e-03 o2o 0e+00
_add("fs100-m4", 4, 512, 8, 100, "gsc_nlms_mw_kernel<4, 1, 2>")  # d 4.3e-02 b2 0.00 nf 0.00 open 1.00 tap 9.8e-03 o2o 0e+00
_add("fs127-m4", 4, 512, 8, 127, "gsc_nlms_mw_kernel<4, 1, 2>")  # d 4.0e-02 b2 0.00 nf 0.00 open 1.00 tap 1.2e-02 o2o 0e+00
_add("fs129-m4", 4, 512, 8, 129, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 4.0e-02 b2 0.00 nf 0.00 open 1.00 tap 8.0e-03 o2o 0e+00
_add("fs191-m4", 4, 512, 8, 191, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 5.2e-02 b2 0.00 nf 0.00 open 1.00 tap 8.6e-03 o2o 0e+00
_add("fs192-m4", 4, 512, 8, 192, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 5.1e-02 b2 0.00 nf 0.00 open 1.00 tap 6.9e-03 o2o 0e+00
_add("fs193-m4", 4, 512, 8, 193, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 4.4e-02 b2 0.00 nf 0.00 open 1.00 tap 8.7e-03 o2o 0e+00
_add("fs255-m4", 4, 512, 8, 255, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 5.2e-02 b2 0.00 nf 0.00 open 1.00 tap 8.2e-03 o2o 0e+00
_add("fs256-m4", 4, 512, 8, 256, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 5.5e-02 b2 0.00 nf 0.00 open 1.00 tap 1.1e-02 o2o 0e+00
_add("fs1-m2", 2, 512, 8, 1, "gsc_nlms_par_kernel<1, 1>", gsc_mu0=4e-4)  # d 2.9e-03 b2 0.00 nf 0.00 open 1.00 tap 6.2e-03 o2o 0e+00
_add("fs65-m2", 2, 512, 8, 65, "gsc_nlms_par_kernel<1, 2>")  # d 1.2e-02 b2 0.00 nf 0.00 open 1.00 tap 7.5e-03 o2o 0e+00
_add("fs129-m2", 2, 512, 8, 129, "gsc_nlms_par_kernel<1, 4>")  # d 1.6e-02 b2 0.00 nf 0.00 open 1.00 tap 6.9e-03 o2o 0e+00
_add("fs256-m2", 2, 512, 8, 256, "gsc_nlms_par_kernel<1, 4>")  # d 2.4e-02 b2 0.00 nf 0.00 open 1.00 tap 8.5e-03 o2o 0e+00
_add("fs1-m10", 10, 512, 6, 1, "gsc_nlms_mw_kernel<8, 2, 1>")  # d 6.7e-03 b2 0.00 nf 0.00 open 1.00 tap 3.9e-03 o2o 0e+00
_add("fs65-m10", 10, 512, 6, 65, "gsc_nlms_mw_kernel<8, 2, 2>")  # d 5.7e-02 b2 0.00 nf 0.00 open 1.00 tap 5.7e-03 o2o 0e+00
_add("fs129-m10", 10, 512, 6, 129, "gsc_nlms_mw_kernel<8, 2, 4>")  # d 8.0e-02 b2 0.00 nf 0.00 open 1.00 tap 5.0e-03 o2o 0e+00
_add("fs256-m10", 10, 512, 6, 256, "gsc_nlms_mw_kernel<8, 2, 4>")  # d 1.1e-01 b2 0.00 nf 0.00 open 1.00 tap 6.3e-03 o2o 0e+00
_add("fs1-m8-serial", 8, 512, 6, 1, "gsc_nlms_kernel<7, 1>", env=SERIAL)  # d 6.8e-03 b2 0.00 nf 0.00 open 1.00 tap 5.6e-03 o2o 0e+00
_add("fs65-m8-serial", 8, 512, 6, 65, "gsc_nlms_kernel<7, 2>", env=SERIAL)  # d 4.3e-02 b2 0.00 nf 0.00 open 1.00 tap 4.0e-03 o2o 0e+00
_add("fs129-m8-serial", 8, 512, 6, 129, "gsc_nlms_kernel<7, 4>", env=SERIAL)  # d 6.4e-02 b2 0.00 nf 0.00 open 1.00 tap 6.1e-03 o2o 0e+00
_add("fs256-m8-serial", 8, 512, 6, 256, "gsc_nlms_kernel<7, 4>", env=SERIAL)  # d 9.1e-02 b2 0.00 nf 0.00 open 1.00 tap 5.7e-03 o2o 0e+00
# ---- every NLMS instantiation chain_decide can select: KPL = 1 / 2 / 4 at filter sizes 48 / 128 / 200; M = 6: five branches over eight wavefronts, 9: one each, 10: nine over eight
_add("inst-m1-fs48", 1, 512, 6, 48, "gsc_nlms_par_kernel<1, 1>")  # d 0.0e+00 b2 0.00 nf 0.00 open 1.00 tap 0.0e+00 o2o 0e+00
_add("inst-m1-fs128", 1, 512, 6, 128, "gsc_nlms_par_kernel<1, 2>")  # d 0.0e+00 b2 0.00 nf 0.00 open 1.00 tap 0.0e+00 o2o 0e+00
_add("inst-m1-fs200", 1, 512, 6, 200, "gsc_nlms_par_kernel<1, 4>")  # d 0.0e+00 b2 0.00 nf 0.00 open 1.00 tap 0.0e+00 o2o 0e+00
_add("inst-m2-fs48", 2, 512, 6, 48, "gsc_nlms_par_kernel<1, 1>")  # d 9.1e-03 b2 0.00 nf 0.00 open 1.00 tap 5.4e-03 o2o 0e+00
_add("inst-m2-fs128", 2, 512, 6, 128, "gsc_nlms_par_kernel<1, 2>")  # d 1.6e-02 b2 0.00 nf 0.00 open 1.00 tap 6.5e-03 o2o 0e+00
_add("inst-m2-fs200", 2, 512, 6, 200, "gsc_nlms_par_kernel<1, 4>")  # d 1.7e-02 b2 0.00 nf 0.00 open 1.00 tap 6.2e-03 o2o 0e+00
_add("inst-m3-fs48", 3, 512, 6, 48, "gsc_nlms_mw_kernel<2, 1, 1>")  # d 1.6e-02 b2 0.00 nf 0.00 open 1.00 tap 5.0e-03 o2o 0e+00
_add("inst-m3-fs128", 3, 512, 6, 128, "gsc_nlms_mw_kernel<2, 1, 2>")  # d 2.3e-02 b2 0.00 nf 0.00 open 1.00 tap 5.9e-03 o2o 0e+00
_add("inst-m3-fs200", 3, 512, 6, 200, "gsc_nlms_mw_kernel<2, 1, 4>")  # d 3.0e-02 b2 0.00 nf 0.00 open 1.00 tap 5.5e-03 o2o 0e+00
_add("inst-m4-fs48", 4, 512, 6, 48, "gsc_nlms_mw_kernel<4, 1, 1>")  # d 2.4e-02 b2 0.00 nf 0.00 open 1.00 tap 5.6e-03 o2o 0e+00
_add("inst-m4-fs128", 4, 512, 6, 128, "gsc_nlms_mw_kernel<4, 1, 2>")  # d 4.0e-02 b2 0.00 nf 0.00 open 1.00 tap 6.8e-03 o2o 0e+00
_add("inst-m4-fs200", 4, 512, 6, 200, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 4.2e-02 b2 0.00 nf 0.00 open 1.00 tap 7.1e-03 o2o 0e+00
_add("inst-m5-fs48", 5, 512, 6, 48, "gsc_nlms_mw_kernel<4, 1, 1>")  # d 2.3e-02 b2 0.00 nf 0.00 open 1.00 tap 4.6e-03 o2o 0e+00
_add("inst-m5-fs128", 5, 512, 6, 128, "gsc_nlms_mw_kernel<4, 1, 2>")  # d 4.2e-02 b2 0.00 nf 0.00 open 1.00 tap 5.0e-03 o2o 0e+00
_add("inst-m5-fs200", 5, 512, 6, 200, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 4.8e-02 b2 0.00 nf 0.00 open 1.00 tap 6.7e-03 o2o 0e+00
_add("inst-m6-fs48", 6, 512, 6, 48, "gsc_nlms_mw_kernel<8, 1, 1>")  # d 3.1e-02 b2 0.00 nf 0.00 open 1.00 tap 5.0e-03 o2o 0e+00
_add("inst-m6-fs128", 6, 512, 6, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 5.0e-02 b2 0.00 nf 0.00 open 1.00 tap 5.7e-03 o2o 0e+00
_add("inst-m6-fs200", 6, 512, 6, 200, "gsc_nlms_mw_kernel<8, 1, 4>")  # d 5.9e-02 b2 0.00 nf 0.00 open 1.00 tap 6.0e-03 o2o 0e+00
_add("inst-m9-fs48", 9, 512, 6, 48, "gsc_nlms_mw_kernel<8, 1, 1>")  # d 4.2e-02 b2 0.00 nf 0.00 open 1.00 tap 6.3e-03 o2o 0e+00
_add("inst-m9-fs128", 9, 512, 6, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 7.0e-02 b2 0.00 nf 0.00 open 1.00 tap 4.4e-03 o2o 0e+00
_add("inst-m9-fs200", 9, 512, 6, 200, "gsc_nlms_mw_kernel<8, 1, 4>")  # d 8.9e-02 b2 0.00 nf 0.00 open 1.00 tap 4.9e-03 o2o 0e+00
_add("inst-m10-fs48", 10, 512, 6, 48, "gsc_nlms_mw_kernel<8, 2, 1>")  # d 4.8e-02 b2 0.00 nf 0.00 open 1.00 tap 5.0e-03 o2o 0e+00
_add("inst-m10-fs128", 10, 512, 6, 128, "gsc_nlms_mw_kernel<8, 2, 2>")  # d 7.6e-02 b2 0.00 nf 0.00 open 1.00 tap 4.5e-03 o2o 0e+00
_add("inst-m10-fs200", 10, 512, 6, 200, "gsc_nlms_mw_kernel<8, 2, 4>")  # d 1.0e-01 b2 0.00 nf 0.00 open 1.00 tap 4.4e-03 o2o 0e+00
_add("inst-m16-fs48", 16, 512, 4, 48, "gsc_nlms_mw_kernel<8, 2, 1>")  # d 5.3e-02 b2 0.00 nf 0.00 open 1.00 tap 4.3e-03 o2o 0e+00
_add("inst-m16-fs128", 16, 512, 4, 128, "gsc_nlms_mw_kernel<8, 2, 2>")  # d 9.2e-02 b2 0.00 nf 0.00 open 1.00 tap 3.7e-03 o2o 0e+00
_add("inst-m16-fs200", 16, 512, 4, 200, "gsc_nlms_mw_kernel<8, 2, 4>")  # d 1.1e-01 b2 0.00 nf 0.00 open 1.00 tap 4.6e-03 o2o 0e+00
_add("inst-m2-fs48-serial", 2, 512, 6, 48, "gsc_nlms_kernel<1, 1>", env=SERIAL)  # d 8.8e-03 b2 0.00 nf 0.00 open 1.00 tap 4.1e-03 o2o 0e+00
_add("inst-m2-fs128-serial", 2, 512, 6, 128, "gsc_nlms_kernel<1, 2>", env=SERIAL)  # d 1.4e-02 b2 0.00 nf 0.00 open 1.00 tap 6.9e-03 o2o 0e+00
_add("inst-m2-fs200-serial", 2, 512, 6, 200, "gsc_nlms_kernel<1, 4>", env=SERIAL)  # d 2.0e-02 b2 0.00 nf 0.00 open 1.00 tap 6.1e-03 o2o 0e+00
_add("inst-m4-fs48-serial", 4, 512, 6, 48, "gsc_nlms_kernel<3, 1>", env=SERIAL)  # d 2.5e-02 b2 0.00 nf 0.00 open 1.00 tap 9.0e-03 o2o 0e+00
_add("inst-m4-fs128-serial", 4, 512, 6, 128, "gsc_nlms_kernel<3, 2>", env=SERIAL)  # d 3.5e-02 b2 0.00 nf 0.00 open 1.00 tap 6.7e-03 o2o 0e+00
_add("inst-m4-fs200-serial", 4, 512, 6, 200, "gsc_nlms_kernel<3, 4>", env=SERIAL)  # d 4.5e-02 b2 0.00 nf 0.00 open 1.00 tap 5.8e-03 o2o 0e+00
_add("inst-m8-fs48-serial", 8, 512, 6, 48, "gsc_nlms_kernel<7, 1>", env=SERIAL)  # d 3.8e-02 b2 0.00 nf 0.00 open 1.00 tap 5.7e-03 o2o 0e+00
_add("inst-m8-fs128-serial", 8, 512, 6, 128, "gsc_nlms_kernel<7, 2>", env=SERIAL)  # d 6.5e-02 b2 0.00 nf 0.00 open 1.00 tap 6.4e-03 o2o 0e+00
_add("inst-m8-fs200-serial", 8, 512, 6, 200, "gsc_nlms_kernel<7, 4>", env=SERIAL)  # d 7.7e-02 b2 0.00 nf 0.00 open 1.00 tap 4.6e-03 o2o 0e+00
_add("inst-m16-fs48-serial", 16, 512, 4, 48, "gsc_nlms_kernel<15, 1>", env=SERIAL)  # d 4.7e-02 b2 0.00 nf 0.00 open 1.00 tap 3.2e-03 o2o 0e+00
_add("inst-m16-fs128-serial", 16, 512, 4, 128, "gsc_nlms_kernel<15, 2>", env=SERIAL)  # d 9.5e-02 b2 0.00 nf 0.00 open 1.00 tap 4.3e-03 o2o 0e+00
_add("inst-m16-fs200-serial", 16, 512, 4, 200, "gsc_nlms_kernel<15, 4>", env=SERIAL)  # d 1.3e-01 b2 0.00 nf 0.00 open 1.00 tap 4.9e-03 o2o 0e+00
# ---- every JACK period: the transforms of the period in front of the NLMS; at hop 64 the rings and the output window span several callbacks
_add("hop64-m8", 8, 64, 64, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 7.9e-02 b2 0.00 nf 0.00 open 1.00 tap 1.4e-02 o2o 0e+00
_add("hop64-m3-fs200", 3, 64, 64, 200, "gsc_nlms_mw_kernel<2, 1, 4>")  # d 3.9e-02 b2 0.00 nf 0.00 open 1.00 tap 9.6e-03 o2o 0e+00
_add("hop128-m8", 8, 128, 32, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 7.2e-02 b2 0.00 nf 0.00 open 1.00 tap 9.8e-03 o2o 0e+00
_add("hop128-m3-fs200", 3, 128, 32, 200, "gsc_nlms_mw_kernel<2, 1, 4>")  # d 3.7e-02 b2 0.00 nf 0.00 open 1.00 tap 7.3e-03 o2o 0e+00
_add("hop256-m8", 8, 256, 16, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 7.2e-02 b2 0.00 nf 0.00 open 1.00 tap 6.9e-03 o2o 0e+00
_add("hop256-m3-fs200", 3, 256, 16, 200, "gsc_nlms_mw_kernel<2, 1, 4>")  # d 3.4e-02 b2 0.00 nf 0.00 open 1.00 tap 7.1e-03 o2o 0e+00
_add("hop1024-m8", 8, 1024, 6, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 9.5e-02 b2 0.00 nf 0.00 open 1.00 tap 8.7e-03 o2o 0e+00
_add("hop1024-m3-fs200", 3, 1024, 6, 200, "gsc_nlms_mw_kernel<2, 1, 4>")  # d 4.4e-02 b2 0.00 nf 0.00 open 1.00 tap 1.2e-02 o2o 0e+00
_add("hop2048-m8", 8, 2048, 3, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 8.1e-02 b2 0.00 nf 0.00 open 1.00 tap 6.5e-03 o2o 0e+00
_add("hop2048-m3-fs200", 3, 2048, 3, 200, "gsc_nlms_mw_kernel<2, 1, 4>")  # d 4.1e-02 b2 0.00 nf 0.00 open 1.00 tap 9.6e-03 o2o 0e+00
_add("hop4096-m8", 8, 4096, 2, 128, "gsc_nlms_mw_kernel<8, 1, 2>")  # d 8.4e-02 b2 0.00 nf 0.00 open 1.00 tap 7.3e-03 o2o 0e+00
_add("hop4096-m3-fs200", 3, 4096, 2, 200, "gsc_nlms_mw_kernel<2, 1, 4>")  # d 3.7e-02 b2 0.00 nf 0.00 open 1.00 tap 8.1e-03 o2o 0e+00
_add("hop64-m5-fs256", 5, 64, 64, 256, "gsc_nlms_mw_kernel<4, 1, 4>")  # d 7.0e-02 b2 0.00 nf 0.00 open 1.00 tap 1.0e-02 o2o 0e+00
# ---- [sample][mic] input
_add("il-m8", 8, 512, 6, 128, "gsc_nlms_mw_kernel<8, 1, 2>", layout=INTERLEAVED)  # d 6.4e-02 b2 0.00 nf 0.00 open 1.00 tap 5.3e-03 o2o 0e+00
_add("il-m3-hop128", 3, 128, 32, 128, "gsc_nlms_mw_kernel<2, 1, 2>", layout=INTERLEAVED)  # d 3.2e-02 b2 0.00 nf 0.00 open 1.00 tap 8.0e-03 o2o 0e+00
# ---- the adaptation gate (thresholds from the oracle's own output-power trace), the second step-size branch, non-finite step sizes
_add("vad-m8", 8, 512, 8, 128, "gsc_nlms_mw_kernel<8, 1, 2>", gsc_use_vad=1, gsc_vad_threshold=0.2034)  # d 4.4e-02 b2 0.00 nf 0.00 open 0.51 tap 3.5e-03 o2o 0e+00
_add("vad-m12", 12, 512, 6, 128, "gsc_nlms_mw_kernel<8, 2, 2>", gsc_use_vad=1, gsc_vad_threshold=0.2018)  # d 5.9e-02 b2 0.00 nf 0.00 open 0.51 tap 5.9e-03 o2o 0e+00
_add("vad-m2", 2, 512, 8, 128, "gsc_nlms_par_kernel<1, 2>", gsc_use_vad=1, gsc_vad_threshold=0.2291)  # d 9.5e-03 b2 0.00 nf 0.00 open 0.50 tap 3.1e-03 o2o 0e+00
_add("mumax-m4", 4, 512, 8, 128, "gsc_nlms_mw_kernel<4, 1, 2>", gsc_mu_max=1.12e-4)  # d 3.6e-02 b2 0.50 nf 0.00 open 1.00 tap 8.1e-03 o2o 0e+00
_add("zeros-m8", 8, 512, 8, 128, "gsc_nlms_mw_kernel<8, 1, 2>", zero=(2, 6))  # d 5.0e-02 b2 0.19 nf 0.19 open 1.00 tap 4.2e-03 o2o 0e+00
# ---- the default kernel and BF_GSC_SERIAL=1 on the same input (the serial halves: fs129-m8-serial above and m16-fs255-serial)
_add("m8-fs129", 8, 512, 6, 129, "gsc_nlms_mw_kernel<8, 1, 4>", input_of="fs129-m8-serial")  # d 6.4e-02 b2 0.00 nf 0.00 open 1.00 tap 6.1e-03 o2o 0e+00
_add("m16-fs255", 16, 512, 4, 255, "gsc_nlms_mw_kernel<8, 2, 4>")  # d 1.3e-01 b2 0.00 nf 0.00 open 1.00 tap 4.6e-03 o2o 0e+00
_add("m16-fs255-serial", 16, 512, 4, 255, "gsc_nlms_kernel<15, 4>", env=SERIAL, input_of="m16-fs255")  # d 1.3e-01 b2 0.00 nf 0.00 open 1.00 tap 4.6e-03 o2o 0e+00
# ---- two streams, cut into batches by test_gsc_gpu.py
_add("carry-m3-fs200-s2", 3, 128, 32, 200, "gsc_nlms_mw_kernel<2, 1, 4>", streams=2)  # d 3.5e-02 b2 0.00 nf 0.00 open 1.00 tap 6.5e-03 o2o 0e+00
# ---- the second step-size branch in the one-wavefront kernel and in the serial one
_add("mumax-m2", 2, 512, 8, 128, "gsc_nlms_par_kernel<1, 2>", gsc_mu_max=1.07e-4)  # d 1.6e-02 b2 0.51 nf 0.00 open 1.00 tap 6.2e-03 o2o 0e+00
_add("mumax-m8-serial", 8, 512, 6, 128, "gsc_nlms_kernel<7, 2>", env=SERIAL, gsc_mu_max=1.15e-4)  # d 5.4e-02 b2 0.51 nf 0.00 open 1.00 tap 4.7e-03 o2o 0e+00


BY_NAME = {c.name: c for c in CASES}
BRANCH2_CASES, ZEROS_CASE = ("mumax-m4", "mumax-m2", "mumax-m8-serial"), "zeros-m8"
VAD_CASES = ("vad-m8", "vad-m12", "vad-m2")


def params(c):
    return make_params("gsc", n_mics=c.M, hop=c.hop, theta=20.0, **c.over)


def scene(c):
    """x [streams][M][F * hop] float32, planar (the GPU tests transpose it for a [sample][mic] handle); c.zero = (first hop, end hop) of a
    stretch of exact zeros on every microphone."""
    x = np.stack([make_scene(c.M, c.F, hop=c.hop, seed=c.seed + 100 * s) for s in range(c.streams)])
    if c.zero:
        x[:, :, c.zero[0] * c.hop:c.zero[1] * c.hop] = 0.0
    return x
