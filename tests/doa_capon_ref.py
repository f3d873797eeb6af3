"""Float64 numpy restatement of the Capon (MVDR) direction-of-arrival map (bf_doa_set_method(BF_DOA_CAPON), include/bfcore.h).
Test infrastructure only.

Frames, spectra X_m(k), the band K and the weights a_d = w(theta_d, k) are doa_ref's (the SRP-PHAT map's).  Per block b and bin k:
  R = sum_{t in block b} X_t X_t^H,  tau = trace R
  tau > 0:  R~ = R / tau + (delta / M) I,  c_d(k) = M / ((1 + delta) a_d^H R~^-1 a_d);  else c_d(k) = 0
  P[b][d] = 1 / |K| sum_{k in K} c_d(k),  peak[b] = argmax_d (the lowest d on ties)
"""
from __future__ import annotations

import numpy as np

import doa_ref
from beamform_amd.synth import mic_delays


def capon_from_spectra(X, a, W: int, delta: float = 1e-3):
    """X [F, M, |K|] complex128 spectra in the band, a [D, M, |K|] weights -> P [F/W, D]."""
    F, M, nK = X.shape
    Xb = X.reshape(F // W, W, M, nK)
    R = np.einsum("bwik,bwjk->bkij", Xb, np.conj(Xb))  # [B, K, M, M]
    tau = np.real(np.einsum("bkii->bk", R))
    ok = tau > 0
    Rt = R / np.where(ok, tau, 1.0)[:, :, None, None] + (delta / M) * np.eye(M)
    av = np.transpose(a, (2, 1, 0))  # [K, M, D]
    sol = np.linalg.solve(Rt, np.broadcast_to(av, (Rt.shape[0],) + av.shape))  # R~^-1 a: [B, K, M, D]
    q = np.real(np.einsum("kmd,bkmd->bkd", np.conj(av), sol))
    c = np.where(ok[:, :, None], M / ((1.0 + delta) * q), 0.0)
    return c.sum(axis=1) / nK


def capon_map(x, mics, hop: int, sr: float, angles, f_lo: float, f_hi: float, W: int, delta: float = 1e-3, hist=None):
    """One stream, planar x [M, F*hop] -> (P [F/W, D] float64, peak [F/W] int)."""
    F = x.shape[1] // hop
    assert F % W == 0
    N = 2 * hop
    K = doa_ref.band_bins(N, sr, f_lo, f_hi)
    assert len(K) > 0
    a = doa_ref.weights(mics, angles, N, sr, K)
    P = np.empty((F // W, len(angles)))
    step = max(1, 256 // W) * W  # frames per pass: whole blocks
    for t0 in range(0, F, step):
        X = doa_ref.spectra(x[:, max(0, (t0 - 1)) * hop:(t0 + step) * hop], hop,
                            hist if t0 == 0 else None)[(1 if t0 > 0 else 0):][:, :, K]
        P[t0 // W:t0 // W + len(X) // W] = capon_from_spectra(X, a, W, delta)
    return P, np.argmax(P, axis=1)


def capon_map_naive(x, mics, hop, sr, angles, f_lo, f_hi, W, delta=1e-3):
    """The definition as a literal loop nest (tiny cases only)."""
    M = x.shape[0]
    F = x.shape[1] // hop
    N = 2 * hop
    win = [np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / N)) for n in range(N)]
    f = doa_ref.frequency_vector(N, sr)
    K = [k for k in range(1, N // 2) if f_lo <= f[k] <= f_hi]
    xs = np.concatenate([np.zeros((M, hop)), x.astype(np.float64)], axis=1)
    P = np.zeros((F // W, len(angles)))
    for b in range(F // W):
        for k in K:
            R = np.zeros((M, M), complex)
            for t in range(b * W, (b + 1) * W):
                X = [sum(xs[m, t * hop + n] * win[n] * np.exp(-2j * np.pi * k * n / N) for n in range(N)) for m in range(M)]
                for i in range(M):
                    for j in range(M):
                        R[i, j] += X[i] * np.conj(X[j])
            tau = sum(R[i, i].real for i in range(M))
            if not tau > 0:
                continue
            Rt = R / tau
            for i in range(M):
                Rt[i, i] += delta / M
            Ri = np.linalg.inv(Rt)
            for d, ang in enumerate(angles):
                tau_m = mic_delays(mics, ang)
                a = [1.0 if m == 0 else np.exp(-2j * np.pi * f[k] * tau_m[m]) for m in range(M)]
                q = sum(np.conj(a[i]) * Ri[i, j] * a[j] for i in range(M) for j in range(M))
                P[b, d] += M / ((1.0 + delta) * q.real)
    return P / len(K)


def srp_and_capon(x, mics, hop, sr, angles, f_lo, f_hi, W, delta=1e-3):
    """Both restatement maps of one scene (the multi-source comparison)."""
    Ps, _ = doa_ref.doa_map(x, mics, hop, sr, angles, f_lo, f_hi, W)
    Pc, _ = capon_map(x, mics, hop, sr, angles, f_lo, f_hi, W, delta)
    return Ps, Pc
