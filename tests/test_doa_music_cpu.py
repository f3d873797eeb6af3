"""MUSIC direction-of-arrival maps and eigenvalue profiles on the host: the float64 restatement (tests/doa_music_ref.py) against its
loop-nest twin, the ranges the definition promises, two-source localisation and the source count on restatement maps, the condition
the GPU cases rely on (a clear cut between the subspaces), the eigensolver of beamform_amd/csrc/doa_eig.hpp compiled here with g++
against numpy.linalg.eigh, and the refusals of the new symbols that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_music_ref as ref  # noqa: E402
import doa_ref  # noqa: E402

from beamform_amd.params import AIRA16_XY  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
GRID2 = np.arange(-180.0, 180.0, 2.0)
BF_EINVAL = -22


def _ang_err(a, b):
    return np.abs((np.asarray(a) - b + 180.0) % 360.0 - 180.0)


# ---- 1. the restatement against the loop nest ------------------------------------------------------------------------------------------
def test_restatement_matches_naive_loops():
    rng = np.random.default_rng(5)
    mics = AIRA16_XY[:3]
    x = rng.standard_normal((3, 4 * 64)).astype(np.float32)
    angles = [-120.0, -90.0, 0.0, 45.0, 170.0]
    for n in (1, 2):
        P, pk, E, gap = ref.music_map(x, mics, 64, SR, angles, 3000.0, 9000.0, 2, n, 0.05)
        Pn, En = ref.music_map_naive(x, mics, 64, SR, angles, 3000.0, 9000.0, 2, n, 0.05)
        assert P.shape == (2, 5) and E.shape == (2, 3) and gap > 1e-3
        assert np.allclose(P, Pn, rtol=1e-12, atol=1e-12) and np.allclose(E, En, rtol=0, atol=1e-12)
        assert np.array_equal(pk, np.argmax(Pn, axis=1))


# ---- 2. ranges ---------------------------------------------------------------------------------------------------------------------------
def test_ranges_profile_and_the_role_of_mu():
    x = make_scene(6, 32, 256, SR, seed=3)
    x[:, 8 * 256:] *= 0.25
    angles = np.arange(-180.0, 180.0, 5.0)
    args = (x, AIRA16_XY[:6], 256, SR, angles, 200.0, 12000.0, 8, 2)
    P, pk, E, _ = ref.music_map(*args, 1e-2)
    assert np.all(P > 0) and np.all(P <= 1.0)
    assert np.all(np.diff(E, axis=1) <= 0) and np.all(E >= 0) and np.all(E <= 1)
    assert np.allclose(E.sum(axis=1), 1.0, rtol=0, atol=1e-12)   # no bin of these blocks has tau = 0
    P2, pk2, E2, _ = ref.music_map(*args, 2e-2)
    assert E2.tobytes() == E.tobytes()
    assert np.array_equal(np.argsort(P, axis=1, kind="stable"), np.argsort(P2, axis=1, kind="stable")) and np.array_equal(pk, pk2)
    # a steering vector as the only frame: it spans the signal subspace, the map is 1 there (nu = 0 in every bin)
    K = doa_ref.band_bins(256, SR, 500.0, 12000.0)
    a = doa_ref.weights(AIRA16_XY[:6], angles, 256, SR, K)
    Pa, Ea, _ = ref.music_from_spectra(a[11][None], a, 1, 1, 1e-2)
    assert abs(Pa[0, 11] - 1.0) <= 1e-12 and np.argmax(Pa[0]) == 11 and np.allclose(Ea[0], [1, 0, 0, 0, 0, 0], atol=1e-12)
    # an all-zero block: nu = 1 and lambda = 0 in every bin
    Pz, Ez, _ = ref.music_from_spectra(np.zeros((2, 6, len(K)), complex), a, 2, 1, 1e-2)
    assert np.all(Pz == 1e-2 / (1e-2 + 1.0)) and not Ez.any()


# ---- 3. two sources, and how many there are --------------------------------------------------------------------------------------------
def test_two_sources_and_the_source_count():
    from beamform_amd.controllers import count_sources, pick_sources
    x = make_scene(8, 32, 512, SR, seed=41, theta_s=20.0, interferers=(-60.0,), sigma_s=0.2, sigma_i=0.05, silent_frac=0.0)
    P, _, E, _ = ref.music_map(x, AIRA16_XY[:8], 512, SR, GRID2, 100.0, 16000.0, 16, 2)
    assert P.shape == (2, 180) and E.shape == (2, 8)
    for b in range(2):
        got = GRID2[pick_sources(P[b], GRID2, 2, 15.0)]
        print("block", b, "picks", got, "profile", E[b][:4], "ratios", E[b][1:4] / E[b][0])
        for src in (20.0, -60.0):
            assert np.min(_ang_err(got, src)) <= 2.0, (b, got)
        assert count_sources(E[b]) == 2
    x1 = make_scene(8, 32, 512, SR, seed=5, interferers=(), silent_frac=0.0)
    _, _, E1, _ = ref.music_map(x1, AIRA16_XY[:8], 512, SR, GRID2, 100.0, 16000.0, 16, 1)
    for b in range(2):
        print("one source, block", b, "profile", E1[b][:4], "ratios", E1[b][1:4] / E1[b][0])
        assert count_sources(E1[b]) == 1
    # the rule itself
    assert count_sources([0.8, 0.19, 0.007, 0.001]) == 2 and count_sources([0.8, 0.19, 0.007, 0.001], rel=0.001) == 3
    assert count_sources([0.8, 0.19, 0.1, 0.05], rel=0.01) == 3 and count_sources([0.8, 0.19, 0.1, 0.05], rel=0.01, n_max=2) == 2
    assert count_sources([1.0, 0.0]) == 1 and count_sources([0.5, 0.5]) == 1 and count_sources([0.6, 0.01, 0.3]) == 1


# ---- 4. the condition the GPU cases rely on --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_case_covariances():
    """Per GPU case and stream: the gap, and the per-bin trace-normalised covariances (what the eigensolver sees)."""
    out = []
    for (M, hop, D, W, layout, S, band, n) in ref.GPU_CASES:
        K = doa_ref.band_bins(2 * hop, SR, *band)
        a = doa_ref.weights(ref.geometry(M), ref.gpu_case_angles(D), 2 * hop, SR, K)
        for s in range(S):
            X = doa_ref.spectra(ref.gpu_case_scene(M, hop, s), hop)[:, :, K]
            _, _, gap = ref.music_from_spectra(X, a, W, n)
            Rn, ok = ref.block_covariances(X, W)
            out.append(((M, hop, D, W, layout, S, band, n, s), gap, Rn[ok]))
    return out


def test_gpu_cases_have_a_clear_cut_between_the_subspaces(gpu_case_covariances):
    for case, gap, _ in gpu_case_covariances:
        print(case, "gap %.3e" % gap)
        assert gap >= 1e-5, (case, gap)


# ---- 5. doa_eig.hpp against eigh -------------------------------------------------------------------------------------------------------
EIG_SRC = r"""
#include <cmath>
#include <vector>
#include "%s"
using namespace bf;
namespace {
struct Mem {  // lower triangle with its diagonal, then V: one matrix in plain memory
    int n;
    std::vector<EigC> a, v;
    explicit Mem(int n_) : n(n_), a(n_ * (n_ + 1) / 2), v(n_ * n_) {}
    double diag(int i) const { return a[i * (i + 1) / 2 + i].re; }
    void set_diag(int i, double x) { a[i * (i + 1) / 2 + i].re = x; }
    EigC low(int i, int c) const { return a[i * (i + 1) / 2 + c]; }
    void set_low(int i, int c, EigC z) { a[i * (i + 1) / 2 + c] = z; }
    EigC vec(int r, int c) const { return v[r * n + c]; }
    void set_vec(int r, int c, EigC z) { v[r * n + c] = z; }
};
template <int N>
struct Reg {  // the register kernels' store: strict lower triangle, real diagonal, V, all plain arrays
    double Rr[N * (N - 1) / 2 + 1], Ri[N * (N - 1) / 2 + 1], Rd[N], Vr[N * N], Vi[N * N];
    double diag(int i) const { return Rd[i]; }
    void set_diag(int i, double x) { Rd[i] = x; }
    EigC low(int i, int c) const { return EigC{Rr[i * (i - 1) / 2 + c], Ri[i * (i - 1) / 2 + c]}; }
    void set_low(int i, int c, EigC z) { Rr[i * (i - 1) / 2 + c] = z.re, Ri[i * (i - 1) / 2 + c] = z.im; }
    EigC vec(int r, int c) const { return EigC{Vr[r * N + c], Vi[r * N + c]}; }
    void set_vec(int r, int c, EigC z) { Vr[r * N + c] = z.re, Vi[r * N + c] = z.im; }
};
template <class S>
double off_over_frob(const S &s, int n) {
    double off = 0, dg = 0;
    for (int i = 0; i < n; ++i) {
        dg += s.diag(i) * s.diag(i);
        for (int c = 0; c < i; ++c) off += 2 * (s.low(i, c).re * s.low(i, c).re + s.low(i, c).im * s.low(i, c).im);
    }
    return off + dg > 0 ? std::sqrt(off / (off + dg)) : 0.0;
}
// A: [n][n][2] row-major; lam [n], V [n][n][2] (column i belongs to lam[i]), rank [n], resid [sweeps]
template <int N, class S>
void run(S &s, int n, const double *A, int sweeps, double *lam, double *V, int *rank, double *resid) {
    for (int i = 0; i < n; ++i) {
        s.set_diag(i, A[(i * n + i) * 2]);
        for (int c = 0; c < i; ++c) s.set_low(i, c, EigC{A[(i * n + c) * 2], A[(i * n + c) * 2 + 1]});
    }
    jacobi_eig<N>(s, n, 0);
    for (int it = 0; it < sweeps; ++it) {
        jacobi_sweep<N>(s, n);
        resid[it] = off_over_frob(s, n);
    }
    for (int i = 0; i < n; ++i) {
        lam[i] = s.diag(i);
        rank[i] = eig_rank<N>(s, n, i);
        for (int c = 0; c < n; ++c) V[(i * n + c) * 2] = s.vec(i, c).re, V[(i * n + c) * 2 + 1] = s.vec(i, c).im;
    }
}
template <int N>
void run_reg(const double *A, int sweeps, double *lam, double *V, int *rank, double *resid) {
    Reg<N> s;
    run<N>(s, N, A, sweeps, lam, V, rank, resid);
}
}  // namespace
// fixed_size: the compile-time path of the register kernels (n = 2, 4, 6, 8); else the run-time path of the memory-resident twin
extern "C" int eig_run(int n, int fixed_size, const double *A, int sweeps, double *lam, double *V, int *rank, double *resid) {
    if (fixed_size) {
        switch (n) {
            case 2: run_reg<2>(A, sweeps, lam, V, rank, resid); return 0;
            case 4: run_reg<4>(A, sweeps, lam, V, rank, resid); return 0;
            case 6: run_reg<6>(A, sweeps, lam, V, rank, resid); return 0;
            case 8: run_reg<8>(A, sweeps, lam, V, rank, resid); return 0;
            default: return -1;
        }
    }
    Mem s(n);
    run<0>(s, n, A, sweeps, lam, V, rank, resid);
    return 0;
}
extern "C" int eig_sweeps(int n) { return jacobi_sweeps(n); }
"""
MAX_SWEEPS = 16


@pytest.fixture(scope="module")
def eig_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("doa_eig")
    src, so = os.path.join(d, "eig.cpp"), os.path.join(d, "libeig.so")
    with open(src, "w") as f:
        f.write(EIG_SRC % os.path.join(ROOT, "beamform_amd", "csrc", "doa_eig.hpp"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-march=native", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.eig_run.argtypes = [C.c_int, C.c_int, dp, C.c_int, dp, dp, ip, dp]

    def run(A, fixed, sweeps=MAX_SWEEPS):
        n = A.shape[0]
        Ac = np.ascontiguousarray(A, np.complex128)
        lam, V = np.empty(n), np.empty((n, n), np.complex128)
        rank, resid = np.empty(n, np.int32), np.empty(sweeps)
        rc = lib.eig_run(n, int(fixed), Ac.ctypes.data_as(dp), sweeps, lam.ctypes.data_as(dp), V.ctypes.data_as(dp),
                         rank.ctypes.data_as(ip), resid.ctypes.data_as(dp))
        assert rc == 0
        return lam, V, rank, resid
    return run, lib.eig_sweeps


def _pinned(R):
    """An odd count's matrix as the register kernels hold it: one more row and column of zeros with -1 on the diagonal."""
    n = R.shape[0]
    A = np.zeros((n + 1, n + 1), complex)
    A[:n, :n] = R
    A[n, n] = -1.0
    return A


def _herm(rng, n, lam):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    A = (q * np.asarray(lam)) @ q.conj().T
    return (A + A.conj().T) / 2


def _eig_set(gpu_case_covariances):
    """(label, matrix, n_sources or None): a few hundred of the GPU cases' per-bin covariances, and the made-up ones."""
    rng = np.random.default_rng(17)
    out = []
    for case, _, Rs in gpu_case_covariances:
        n = case[7]
        for R in Rs[rng.choice(len(Rs), size=min(len(Rs), 24), replace=False)]:
            out.append((case, R, n))
    for n in (2, 3, 8, 9, 16, 32):
        v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        out.append(("rank 1", np.outer(v, v.conj()) / np.vdot(v, v).real, 1))
        out.append(("identity", np.eye(n, dtype=complex) / n, None))       # no cut anywhere: eigenvalues only
        X = rng.standard_normal((n, 2 * n)) + 1j * rng.standard_normal((n, 2 * n))
        R = X @ X.conj().T
        out.append(("full rank", R / np.trace(R).real, max(1, n // 3)))
        if n >= 3:
            # two equal eigenvalues, both on the signal side of the cut (n = 2) and, for the larger sizes, two more on the noise side
            lam = np.concatenate([[0.3, 0.3], np.linspace(0.1, 0.01, n - 2)])
            if n >= 8:
                lam[-2] = lam[-1]
            out.append(("equal pair", _herm(rng, n, lam / lam.sum()), 2))
    return out


def test_doa_eig_hpp_matches_eigh(eig_lib, gpu_case_covariances):
    run, sweeps_of = eig_lib
    worst = {}   # (n, fixed) -> per-sweep maximum of the residue
    n_done = 0
    for label, R, n_src in _eig_set(gpu_case_covariances):
        M = R.shape[0]
        variants = [(R, False)]
        if M <= 8:
            variants.append((R if M % 2 == 0 else _pinned(R), True))
        for A, fixed in variants:
            n = A.shape[0]
            lam, V, rank, resid = run(A, fixed)
            key = (n, fixed)
            worst[key] = np.maximum(worst.get(key, 0.0), resid)
            # the committed count: residue below 1e-14 one sweep earlier, and the results taken at exactly that count
            ns = sweeps_of(n)
            assert ns <= MAX_SWEEPS and resid[ns - 2] < 1e-14, (label, n, fixed, resid)
            lam, V, rank, _ = run(A, fixed, ns)
            w, U = np.linalg.eigh(A)
            w, U = w[::-1], U[:, ::-1]
            assert sorted(rank.tolist()) == list(range(n))
            by_rank = np.empty(n)
            by_rank[rank] = lam
            assert np.all(np.diff(by_rank) <= 0)
            assert np.max(np.abs(by_rank - w)) <= 1e-12, (label, n, fixed, np.max(np.abs(by_rank - w)))
            assert np.linalg.norm(V.conj().T @ V - np.eye(n)) <= 1e-12
            if n_src is not None:
                noise = rank >= n_src
                Pn = V[:, noise] @ V[:, noise].conj().T
                Pr = U[:, n_src:] @ U[:, n_src:].conj().T
                assert np.linalg.norm(Pn - Pr) <= 1e-10, (label, n, fixed, np.linalg.norm(Pn - Pr))
            if fixed and M % 2 == 1:   # the pinned row sorts last, stays e_M, and mixes into nothing
                assert rank[M] == M and lam[M] == -1.0 and V[M, M] == 1.0 and not V[M, :M].any() and not V[:M, M].any()
            n_done += 1
    assert n_done > 300
    needed = {True: 0, False: 0}   # sizes up to 8 / above: the first sweep after which every member is below 1e-14
    for (n, fixed), r in sorted(worst.items()):
        first = int(np.argmax(r < 1e-14)) + 1
        needed[n <= 8] = max(needed[n <= 8], first)
        print("size %2d %s: worst residue per sweep %s -> below 1e-14 after %d" %
              (n, "fixed  " if fixed else "runtime", " ".join("%.1e" % v for v in r[:12]), first))
    # the committed counts are the smallest that do, plus one
    assert sweeps_of(8) == needed[True] + 1 and sweeps_of(32) == needed[False] + 1, (needed, sweeps_of(8), sweeps_of(32))


# ---- 6. the surface, and the refusals that need no device ------------------------------------------------------------------------------
def test_symbols_declared_listed_exported_and_null_handle_refused():
    from beamform_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "bfcore.h")).read()
    declared = set(re.findall(r"\b(bf_[a-z_0-9]+)\s*\(", header))
    for name in ("bf_doa_set_sources", "bf_doa_set_music_floor", "bf_doa_process_device_eig", "bf_doa_process_eig"):
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert re.search(r"BF_DOA_MUSIC\s*=\s*2", header) and capi.BF_DOA_MUSIC == 2
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    assert lib.bf_doa_set_sources(None, 1) == BF_EINVAL          # no device is touched
    assert lib.bf_doa_set_music_floor(None, 1e-2) == BF_EINVAL
    assert lib.bf_doa_set_method(None, capi.BF_DOA_MUSIC) == BF_EINVAL
    assert lib.bf_doa_process_device_eig(None, p, 4, p, p, p, None) == BF_EINVAL
    assert lib.bf_doa_process_eig(None, p, 4, p, p, p) == BF_EINVAL
