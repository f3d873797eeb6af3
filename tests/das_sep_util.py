"""Shared by the CPU and the GPU tests of the frame-pair kernels' delay-structured gains (geometry.hpp das_sep_gains_w64_f64): the CPU
restatement under tests/host_emul_sep (built here with g++ on first use), and the figure both tests hang on."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# New form against table form on the CPU (EXPERIMENTS.md, "Delay-structured gains"): the largest deviation of the backward transform's
# output in double, relative to the largest magnitude of the frame pair's output, over the geometries, look angles and scenes of
# tests/test_das_sep_cpu.py -- which asserts that the figure still holds.  The GPU test allows 4 x this between the kernel and the CPU
# restatement of the new form.
SEP_VS_TABLE_BOUND = 5.0e-15   # measured: 4.0e-15 at most (per bin of the summed spectrum, relative to its peak: 9.5e-15)

GEOMETRIES = {
    # tests/test_fused_bins_gpu.py's merge test: the default 8 microphones (1 = 7), no coinciding microphones, one merged pair of two
    "aira16-first-8 (1 = 7)": None,
    "all distinct": [(0.158, 0.115), (0.158, -0.115), (-0.045, 0.0), (-0.05, -0.188), (-0.195, 0.0), (-0.057, 0.186), (0.18, 0.0), (0.056, -0.171)],
    "2 = 3 and 5 = 6": [(0.0, 0.0), (0.1, 0.02), (-0.05, 0.12), (-0.05, 0.12), (0.07, -0.11), (0.13, 0.09), (0.13, 0.09), (-0.2, 0.0)],
    "symmetric about theta = 0": [(0.0, 0.0), (0.1, 0.07), (0.1, -0.07), (-0.12, 0.03), (-0.12, -0.03), (0.2, 0.0)],
}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def load_sep_lib():
    d = os.path.join(ROOT, "tests", "host_emul_sep")
    so, src = os.path.join(d, "libemul_sep.so"), os.path.join(d, "emul_sep.cpp")
    deps = [src, os.path.join(ROOT, "tests", "host_emul", "emul.cpp")] + [os.path.join(ROOT, "beamform_amd", "csrc", h) for h in ("geometry.hpp", "das_f64_plan.hpp", "fft1024_w64.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.emul_sep_check.restype = None
    lib.emul_sep_das.restype = None
    return lib


def xy(p):
    return np.array([m[0] for m in p["mics"]], np.float64), np.array([m[1] for m in p["mics"]], np.float64)


def sep_check(lib, p, theta, perturb=(-1, 0, 0.0)):
    """dict(ok, bound, worst, e512, e513, d511, path) of the host's check for the table of look angle `theta`."""
    mx, my = xy(p)
    out = np.zeros(8)
    lib.emul_sep_check(len(mx), C.c_double(float(p["sample_rate"])), ptr(mx), ptr(my), C.c_double(theta), int(perturb[0]), int(perturb[1]), C.c_double(perturb[2]), ptr(out))
    return dict(ok=bool(out[0]), bound=out[1], worst=out[2], e512=bool(out[3]), e513=bool(out[4]), d511=out[5], d511_kernel=out[7], path=int(out[6]))


def sep_das(lib, p, theta, x, form, want_u=False, want_U=False):
    """(y float32 [F * 512], u, U): the restated kernel on planar x [M][F * 512]; u / U complex [pairs][1024] or None."""
    mx, my = xy(p)
    M, F = x.shape[0], x.shape[1] // 512
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty(F * 512, np.float32)
    P = (F + 1) // 2
    u = np.zeros((P, 1024), np.complex128) if want_u else None
    U = np.zeros((P, 1024), np.complex128) if want_U else None
    lib.emul_sep_das(M, C.c_double(float(p["sample_rate"])), ptr(mx), ptr(my), C.c_double(theta), ptr(x), C.c_long(F), int(form), ptr(y),
                     ptr(u) if want_u else None, ptr(U) if want_U else None)
    return y, u, U
