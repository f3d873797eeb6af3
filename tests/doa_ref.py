"""Float64 numpy restatement of the direction-of-arrival map (bf_doa_*, include/bfcore.h).  Test infrastructure only.

P[s][b][d] = 1 / (W |K| M^2) sum_{t in block b} sum_{k in K} | sum_m conj(w_m(theta_d, k)) X^_{s,m,t}(k) |^2
with frames [hop t-1 | hop t] x periodic sqrt-Hann (hop -1 = zeros at a cold start), X^ = X / |X| where |X| > eps else 0, the band K
among bins 1 .. N/2-1 on das's frequency vector (quirk Q1: f[N/2-1] = sr/2) and das's weights exp(-i 2 pi f_k tau_m(theta)), tau_0 = 0.
"""
from __future__ import annotations

import numpy as np

from beamform_amd.synth import mic_delays


def frequency_vector(n_fft: int, sr: float) -> np.ndarray:
    f = np.zeros(n_fft)
    k = np.arange(1, n_fft // 2)
    f[k] = k / n_fft * sr
    f[n_fft - k] = -k / n_fft * sr
    f[n_fft // 2 - 1] = sr / 2
    return f


def band_bins(n_fft: int, sr: float, f_lo: float, f_hi: float) -> np.ndarray:
    f = frequency_vector(n_fft, sr)
    k = np.arange(1, n_fft // 2)
    return k[(f[k] >= f_lo) & (f[k] <= f_hi)]


def weights(mics, angles, n_fft: int, sr: float, bins) -> np.ndarray:
    """w [D, M, |K|] complex128: das's steering column (update_weights(true)) for every angle."""
    f = frequency_vector(n_fft, sr)[bins]
    w = np.empty((len(angles), len(mics), len(bins)), np.complex128)
    for d, a in enumerate(angles):
        tau = mic_delays(mics, a)
        w[d] = np.exp(-2j * np.pi * f[None, :] * tau[:, None])
        w[d, 0] = 1.0
    return w


def spectra(x: np.ndarray, hop: int, hist: np.ndarray = None) -> np.ndarray:
    """x [M, F*hop] float32 (one stream, planar) -> X [F, M, N] complex128 of the windowed frames."""
    M = x.shape[0]
    F = x.shape[1] // hop
    N = 2 * hop
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))
    prev = np.zeros((M, hop)) if hist is None else np.asarray(hist, np.float64)
    xx = np.concatenate([prev, x.astype(np.float64)], axis=1)
    idx = np.arange(F)[:, None] * hop + np.arange(N)[None, :]
    frames = xx[:, idx].transpose(1, 0, 2) * win  # [F, M, N]
    return np.fft.fft(frames, axis=-1)


def doa_map(x, mics, hop: int, sr: float, angles, f_lo: float, f_hi: float, W: int, eps: float = 1e-10, hist=None):
    """One stream, planar x [M, F*hop] -> (P [F/W, D] float64, peak [F/W] int)."""
    M = x.shape[0]
    F = x.shape[1] // hop
    assert F % W == 0
    N = 2 * hop
    K = band_bins(N, sr, f_lo, f_hi)
    assert len(K) > 0
    w = np.conj(weights(mics, angles, N, sr, K))  # [D, M, K]
    Pt = np.empty((F, len(angles)))
    step = max(1, int(2e7 // (len(angles) * len(K) * 16)))
    for t0 in range(0, F, step):
        X = spectra(x[:, max(0, (t0 - 1)) * hop:(t0 + step) * hop], hop,
                    hist if t0 == 0 else None)[(1 if t0 > 0 else 0):][:, :, K]
        mag = np.abs(X)
        Xh = np.where(mag > eps, X / np.where(mag > eps, mag, 1.0), 0.0)
        y = np.einsum("dmk,tmk->tdk", w, Xh)
        Pt[t0:t0 + len(Xh)] = np.sum(y.real ** 2 + y.imag ** 2, axis=-1)
    P = Pt.reshape(F // W, W, len(angles)).sum(axis=1) / (W * len(K) * M * M)
    return P, np.argmax(P, axis=1)


def doa_map_naive(x, mics, hop, sr, angles, f_lo, f_hi, W, eps=1e-10):
    """The definition as a literal loop nest (tiny cases only)."""
    M = x.shape[0]
    F = x.shape[1] // hop
    N = 2 * hop
    win = [np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / N)) for n in range(N)]
    f = frequency_vector(N, sr)
    K = [k for k in range(1, N // 2) if f_lo <= f[k] <= f_hi]
    xs = np.concatenate([np.zeros((M, hop)), x.astype(np.float64)], axis=1)
    P = np.zeros((F // W, len(angles)))
    for t in range(F):
        Xh = {}
        for m in range(M):
            fr = [xs[m, t * hop + n] * win[n] for n in range(N)]
            for k in K:
                X = sum(fr[n] * np.exp(-2j * np.pi * k * n / N) for n in range(N))
                Xh[m, k] = X / abs(X) if abs(X) > eps else 0.0
        for d, a in enumerate(angles):
            tau = mic_delays(mics, a)
            for k in K:
                y = 0j
                for m in range(M):
                    wm = 1.0 if m == 0 else np.exp(-2j * np.pi * f[k] * tau[m])
                    y += np.conj(wm) * Xh[m, k]
                P[t // W, d] += abs(y) ** 2
    return P / (W * len(K) * M * M)
