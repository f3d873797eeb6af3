"""numpy restatement of gss.cpp:110-146 that keeps EVERY separated source (test infrastructure).

The reference computes this_yf = sep_matrix[j] * in_fft.col(j) per frame and bin and emits only this_yf(0) (gss.cpp:120-121).  Here row r of
the output is this_yf(r): in band with the gate open (sep_matrix[j] x)(r) for r < S; gate closed 0.01 X_0 for r = 0 and 0 above
(gss.cpp:139-141); out of band and r >= S zero.  Every row takes the same backward transform, window, out_amp and overlap-add
(oracle.np_oracle.istft_ola) with its own tail.

order = "blas": the expressions of oracle.np_oracle.gss_bins, bin by bin, so row 0 is that function's output bit for bit.
order = "serial" / "pairwise": the sums over the microphones spelled out, m = 0, 1, ... or as a balanced tree (what DPP butterflies over
the lanes of a group compute), vectorised over the bins -- two roundings of the same recursion, to bound its rounding floor.
"""
import numpy as np

from oracle import np_oracle


def _sum_mics(terms, order):
    if order == "serial":
        acc = terms[0]
        for t in terms[1:]:
            acc = acc + t
        return acc
    n = 1
    while n < len(terms):
        n *= 2
    v = list(terms) + [np.zeros_like(terms[0])] * (n - len(terms))
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


class _Demixer:
    """sep_matrix of every bin and its update (gss.cpp:110-146)."""

    def __init__(self, p, N, order):
        self.p, self.N, self.order = p, N, order
        f = np.abs(np_oracle.freq_vector(N, p["sample_rate"]))
        self.idx = np.nonzero((f >= p["freq_min"]) & (f <= p["freq_max"]))[0]

    def restart(self, C):
        """sep_matrix[j] = weights[j].adjoint() (gss.cpp:90-93).  C: [N, M, S]"""
        self.C = C
        self.S = C.shape[2]
        self.W = np.conj(np.transpose(C, (0, 2, 1))).copy()  # [N, S, M]
        self.Ch = self.W.copy()

    def frame(self, x, Yt):
        """x [M, N] -> Yt [R, N] (zeros on entry)."""
        if self.order == "blas":
            self._frame_blas(x, Yt)
        else:
            self._frame_ordered(x, Yt)

    def _frame_blas(self, x, Yt):
        p, S, W, C, Ch = self.p, self.S, self.W, self.C, self.Ch
        M, N = x.shape
        R = Yt.shape[0]
        c2 = 2 * (1 // S)  # integer division, quirk Q13
        mu, lam = p["mu"], p["lambda_"]
        mag = np.abs(x).sum(axis=0) / (M * N)
        for j in self.idx:
            if mag[j] > p["freq_mag_threshold"]:
                xj = x[:, j]
                y = W[j] @ xj
                Yt[:min(R, S), j] = y[:R]
                E = np.outer(y, y.conj())
                np.fill_diagonal(E, 0)
                alpha = (np.abs(xj) ** 2).sum() ** 2
                dj1 = 4 * S * (1 / alpha) * np.outer(E @ y, xj.conj())
                dj2 = c2 * ((W[j] @ C[j]) - np.eye(S)) @ Ch[j]
                W[j] = (1 - lam * mu) * W[j] - mu * (dj1 + dj2)
            else:
                Yt[0, j] = 0.01 * x[0, j]

    def _frame_ordered(self, x, Yt):
        p, S, idx, order = self.p, self.S, self.idx, self.order
        M, N = x.shape
        R = Yt.shape[0]
        c2 = 2 * (1 // S)
        mu, lam = p["mu"], p["lambda_"]
        xs = x[:, idx]                                   # [M, nb]
        W = self.W[idx]                                  # [nb, S, M]
        mag = _sum_mics([np.abs(xs[m]) for m in range(M)], order) / (M * N)
        gate = mag > p["freq_mag_threshold"]
        y = [_sum_mics([W[:, r, m] * xs[m] for m in range(M)], order) for r in range(S)]
        alpha = _sum_mics([xs[m].real ** 2 + xs[m].imag ** 2 for m in range(M)], order) ** 2
        with np.errstate(all="ignore"):
            c1 = 4 * S * (1 / alpha)
            Wn = np.empty_like(W)
            if c2:  # only S == 1: dj2 = 2 (W C - I) C^H
                Cj = self.C[idx]                         # [nb, M, 1]
                wc = _sum_mics([W[:, 0, k] * Cj[:, k, 0] for k in range(M)], order) - 1.0
            for r in range(S):
                Ey = np.zeros_like(y[0])
                for r2 in range(S):
                    if r2 != r:
                        Ey = Ey + (y[r] * np.conj(y[r2])) * y[r2]
                for m in range(M):
                    d = (Ey * np.conj(xs[m])) * c1
                    if c2:
                        d = d + (wc * np.conj(Cj[:, m, 0])) * c2
                    Wn[:, r, m] = W[:, r, m] * (1 - lam * mu) - d * mu
        self.W[idx[gate]] = Wn[gate]
        for r in range(min(R, S)):
            Yt[r, idx] = np.where(gate, y[r], 0.01 * xs[0] if r == 0 else 0.0)


def gss_sources(p, x, segments, R, order="blas"):
    """x [M, F*H] float32 from a cold start, cut into segments (n_frames, C or None): C is the [N, M, S] constraint matrix of
    oracle.OracleNode.weights() after the control call in front of the segment (a non-None C restarts sep_matrix = C^H; the first
    segment needs one).  -> (y [R, F*H] float32, Y [R, F, N] complex128)."""
    assert order in ("blas", "serial", "pairwise")
    X = np_oracle.stft(p, x)                             # [F, M, N]
    F, M, N = X.shape
    assert sum(n for n, _ in segments) == F and segments[0][1] is not None
    Y = np.zeros((R, F, N), np.complex128)
    dm = _Demixer(p, N, order)
    t = 0
    for n, C in segments:
        if C is not None:
            dm.restart(np.array(C, np.complex128))
        for _ in range(n):
            Yt = np.zeros((R, N), np.complex128)
            dm.frame(X[t], Yt)
            Y[:, t] = Yt
            t += 1
    y = np.stack([np_oracle.istft_ola(p, Y[r], p["out_amp"]) for r in range(R)])
    return y, Y


def circle_mics(n, radius=0.2):
    """n microphones on a circle (more than the 16 of beamform_amd.params.AIRA16_XY)."""
    a = 2 * np.pi * np.arange(n) / n
    return [(float(radius * np.cos(v)), float(radius * np.sin(v))) for v in a]
