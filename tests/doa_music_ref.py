"""Float64 numpy restatement of the MUSIC direction-of-arrival map and its eigenvalue profile (bf_doa_set_method(BF_DOA_MUSIC),
include/bfcore.h).  Test infrastructure only.

Frames, spectra X_m(k), the band K and the weights a_d = w(theta_d, k) are doa_ref's (the SRP-PHAT map's).  Per block b and bin k:
  R = sum_{t in block b} X_t X_t^H,  tau = trace R
  tau > 0:  R / tau = sum_i lambda_i v_i v_i^H (lambda descending),  nu_d(k) = 1 / M sum_{i > n} |v_i^H a_d|^2;  else nu_d(k) = 1, lambda = 0
  P[b][d] = mu / (mu + 1 / |K| sum_{k in K} nu_d(k)),  peak[b] = argmax_d (the lowest d on ties)
  E[b][i] = 1 / |K| sum_{k in K} lambda_i(k)
"""
from __future__ import annotations

import numpy as np

import doa_ref
from beamform_amd.synth import mic_delays


SR = 48000.0
FULL = (100.0, 16000.0)  # the band of the Capon tests
# The cases of test_doa_music_gpu.py's map test; test_doa_music_cpu.py checks the condition they rely on (gap >= 1e-5).
GPU_CASES = [  # M, hop, D, W, layout, streams, band, n
    (2, 128, 72, 4, 0, 1, FULL, 1),
    (3, 512, 72, 8, 1, 3, FULL, 1),                  # an odd count: the pinned partner row
    (8, 512, 360, 8, 0, 3, (100.0, 24000.0), 2),
    (8, 512, 1, 4, 0, 1, (300.0, 2000.0), 2),        # |K| < 64: one partly filled wavefront
    (6, 512, 72, 4, 0, 1, FULL, 2),                  # W < M: a rank-deficient covariance
    (9, 512, 72, 8, 1, 1, FULL, 2),                  # an odd count above 8
    (16, 2048, 72, 8, 0, 1, (300.0, 8000.0), 3),
    (32, 128, 8, 16, 0, 1, FULL, 3),
]
GPU_FRAMES = 32


def geometry(M: int):
    """test_doa_capon_gpu.py's arrays: the first M of the 16-microphone array, two rings of 16 above that."""
    from beamform_amd.params import AIRA16_XY
    if M <= 16:
        return list(AIRA16_XY[:M])
    ring = [(0.1 * np.cos(2 * np.pi * i / 16), 0.1 * np.sin(2 * np.pi * i / 16)) for i in range(16)] + \
           [(0.2 * np.cos(2 * np.pi * (i + 0.5) / 16), 0.2 * np.sin(2 * np.pi * (i + 0.5) / 16)) for i in range(16)]
    return ring[:M]


def gpu_case_scene(M: int, hop: int, s: int):
    """Stream s of a GPU case (test_doa_capon_gpu.py's scenes)."""
    from beamform_amd.synth import make_scene
    return make_scene(M, GPU_FRAMES, hop, SR, seed=100 + s, mics=geometry(M), theta_s=-40.0 + 50 * s)


def gpu_case_angles(D: int):
    return np.linspace(-180.0, 180.0, D, endpoint=False) + 0.25


def block_covariances(X, W: int):
    """X [F, M, |K|] -> (R / tau [B, K, M, M], ok [B, K]); R / tau is 0 where tau = 0."""
    F, M, nK = X.shape
    Xb = X.reshape(F // W, W, M, nK)
    R = np.einsum("bwik,bwjk->bkij", Xb, np.conj(Xb))
    tau = np.real(np.einsum("bkii->bk", R))
    ok = tau > 0
    return R / np.where(ok, tau, 1.0)[:, :, None, None], ok


def music_from_spectra(X, a, W: int, n: int, mu: float = 1e-2):
    """X [F, M, |K|] complex128 spectra in the band, a [D, M, |K|] weights -> (P [F/W, D], E [F/W, M], gap).
    gap: the minimum over blocks and bins (with tau > 0) of (lambda_n - lambda_{n+1}) / lambda_1."""
    F, M, nK = X.shape
    assert 1 <= n <= M - 1
    Rn, ok = block_covariances(X, W)
    lam, V = np.linalg.eigh(Rn)              # ascending
    lam, V = lam[..., ::-1], V[..., ::-1]    # descending: column i belongs to lam[i]
    lam = np.where(ok[:, :, None], np.maximum(lam, 0.0), 0.0)
    av = np.transpose(a, (2, 1, 0))          # [K, M, D]
    y = np.einsum("bkmi,kmd->bkid", np.conj(V[..., n:]), av)   # v_i^H a_d for the noise vectors
    nu = np.sum(y.real ** 2 + y.imag ** 2, axis=2) / M
    nu = np.where(ok[:, :, None], nu, 1.0)
    P = mu / (mu + nu.sum(axis=1) / nK)
    E = lam.sum(axis=1) / nK
    g = (lam[..., n - 1] - lam[..., n]) / np.where(ok, lam[..., 0], 1.0)
    gap = float(np.min(g[ok])) if ok.any() else float("inf")
    return P, E, gap


def music_map(x, mics, hop: int, sr: float, angles, f_lo: float, f_hi: float, W: int, n: int = 1, mu: float = 1e-2, hist=None):
    """One stream, planar x [M, F*hop] -> (P [F/W, D] float64, peak [F/W] int, E [F/W, M] float64, gap)."""
    F = x.shape[1] // hop
    assert F % W == 0
    N = 2 * hop
    K = doa_ref.band_bins(N, sr, f_lo, f_hi)
    assert len(K) > 0
    a = doa_ref.weights(mics, angles, N, sr, K)
    P = np.empty((F // W, len(angles)))
    E = np.empty((F // W, x.shape[0]))
    gap = float("inf")
    step = max(1, 256 // W) * W  # frames per pass: whole blocks
    for t0 in range(0, F, step):
        X = doa_ref.spectra(x[:, max(0, (t0 - 1)) * hop:(t0 + step) * hop], hop,
                            hist if t0 == 0 else None)[(1 if t0 > 0 else 0):][:, :, K]
        b0, nb = t0 // W, len(X) // W
        P[b0:b0 + nb], E[b0:b0 + nb], g = music_from_spectra(X, a, W, n, mu)
        gap = min(gap, g)
    return P, np.argmax(P, axis=1), E, gap


def music_map_naive(x, mics, hop, sr, angles, f_lo, f_hi, W, n=1, mu=1e-2):
    """The definition as a literal loop nest (tiny cases only) -> (P, E)."""
    M = x.shape[0]
    F = x.shape[1] // hop
    N = 2 * hop
    win = [np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * j / N)) for j in range(N)]
    f = doa_ref.frequency_vector(N, sr)
    K = [k for k in range(1, N // 2) if f_lo <= f[k] <= f_hi]
    xs = np.concatenate([np.zeros((M, hop)), x.astype(np.float64)], axis=1)
    nu = np.zeros((F // W, len(angles)))
    E = np.zeros((F // W, M))
    for b in range(F // W):
        for k in K:
            R = np.zeros((M, M), complex)
            for t in range(b * W, (b + 1) * W):
                X = [sum(xs[m, t * hop + j] * win[j] * np.exp(-2j * np.pi * k * j / N) for j in range(N)) for m in range(M)]
                for i in range(M):
                    for j in range(M):
                        R[i, j] += X[i] * np.conj(X[j])
            tau = sum(R[i, i].real for i in range(M))
            if not tau > 0:
                nu[b] += 1.0
                continue
            lam, V = np.linalg.eigh(R / tau)
            order = sorted(range(M), key=lambda i: -lam[i])
            for slot, i in enumerate(order):
                E[b, slot] += max(lam[i], 0.0)
            for d, ang in enumerate(angles):
                tau_m = mic_delays(mics, ang)
                a = [1.0 if m == 0 else np.exp(-2j * np.pi * f[k] * tau_m[m]) for m in range(M)]
                for i in order[n:]:
                    nu[b, d] += abs(sum(np.conj(V[m, i]) * a[m] for m in range(M))) ** 2 / M
    return mu / (mu + nu / len(K)), E / len(K)
