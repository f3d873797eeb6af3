"""numpy restatement of gss's multi-source post-filter (bf_config.gss_postfilter; test infrastructure).

Every live row r < min(S_t, R) of a frame is replaced by the output of the reference's MPF block (phasempf.cpp:140-191, 254-295) with
soi = the row and int2 = the sum of the other live rows' |.|^2 in ascending row order.  The block is spelled with the expressions of
oracle.np_oracle.phasempf_bins (lines 217-248), so that fed with phasempf's soi / inter pair and out_amp = 1 row 0 is that function's
output bit for bit (tests/test_gss_postfilter_cpu.py).  out_amp is NOT applied here: gss's backward path applies it to every row.
Rows r >= min(S_t, R) are left as they are and their state does not advance.  Vectorised over the bins, serial over the frames.
"""
import numpy as np


class _RowState:
    def __init__(self, N):
        self.Sprev = np.zeros(N); self.Stmp = np.zeros(N); self.Smin = np.zeros(N); self.lam = np.zeros(N)
        self.Z = np.zeros(N); self.rev0 = np.zeros(N); self.rev1 = np.zeros(N)
        self.cL, self.firstL = 0, True


def _mpf_block(p, st, soi, int2, taps):
    """One frame of one row: soi [N] complex, int2 [N] (index 0 already 0) -> the filtered row [N]."""
    aS, aD, aD2, delta, L = p["mcra_alphaS"], p["mcra_alphaD"], p["mcra_alphaD2"], p["mcra_delta"], p["mcra_L"]
    N = soi.shape[0]
    soi2 = np.abs(soi) ** 2
    soi2[0] = 0.0
    Sf = taps * soi2
    Sf[0] = np.abs(soi[0])
    S = aS * st.Sprev + (1 - aS) * Sf
    if st.cL > L:
        st.Smin = np.minimum(st.Stmp, S); st.Stmp = S.copy(); st.cL = 1; st.firstL = False
    else:
        st.Smin = np.minimum(st.Smin, S); st.Stmp = np.minimum(st.Stmp, S); st.cL += 1
    cond = (S < st.Smin * delta) | (st.lam > soi2)
    if st.firstL:
        cond = np.ones(N, bool)
    if st.firstL and (1.0 / st.cL) > aD:
        new = (1.0 / st.cL) * st.lam + (1.0 - 1.0 / st.cL) * soi2
    else:
        new = aD2 * st.lam + (1.0 - aD) * soi2
    st.lam = np.where(cond, new, st.lam)
    st.Sprev = S
    st.Z = p["mpf_alphaS"] * st.Z + (1 - p["mpf_alphaS"]) * int2
    k = 1 - p["mpf_rev_gamma"] / p["mpf_rev_delta"]
    st.rev0 = p["mpf_rev_gamma"] * st.rev0 + k * soi2
    st.rev1 = p["mpf_rev_gamma"] * st.rev1 + k * int2
    Lam = np.sqrt(st.lam + p["mpf_eta"] * st.Z + st.rev0 + st.rev1)
    ph = np.angle(soi)
    if p["out_only_noise"]:
        g = Lam
    else:
        g = np.abs(soi) - (np.sqrt(st.lam) if p["out_only_mcra"] else Lam)
        g = np.where(g < 0, p["noise_floor"], g)
    Yt = g * np.cos(ph) + 1j * (g * np.sin(ph))
    Yt[0] = 0.0
    return Yt


def postfilter(p, Y, sources_per_frame):
    """Y [R, F, N] complex128: the rows of one beam from a cold start (tests/gss_sources_ref.py gss_sources).  sources_per_frame: S_t,
    one int for the whole stream or one per frame.  -> the filtered rows [R, F, N]."""
    Y = np.asarray(Y, np.complex128)
    R, F, N = Y.shape
    S_t = np.broadcast_to(np.asarray(sources_per_frame, int), (F,))
    taps = np.ones(N); taps[1] = 0.75; taps[N - 1] = 0.75
    states = [_RowState(N) for _ in range(R)]
    out = Y.copy()
    for t in range(F):
        live = min(int(S_t[t]), R)
        n2 = [np.abs(Y[r, t]) ** 2 for r in range(live)]
        for r in range(live):
            int2 = np.zeros(N)
            for r2 in range(live):
                if r2 != r:
                    int2 = int2 + n2[r2]
            int2[0] = 0.0
            out[r, t] = _mpf_block(p, states[r], Y[r, t], int2, taps)
    return out
