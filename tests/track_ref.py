"""Restatements for the steering-track tests (bf_track_*, include/bfcore.h).  Test infrastructure only.

oracle_tracked: the reference node with /theta messages landing between callbacks -- the oracle driven hop by hop, set_theta called in
front of hop t whenever the angle in force changes.  from_peaks: the numpy statement of bf_track_from_peaks_device."""
import numpy as np


def angle_in_force(angles, idx, theta0):
    """The index rule: 0 .. len(angles)-1 names a candidate angle, anything else the handle's own theta."""
    i = int(idx)
    return float(angles[i]) if 0 <= i < len(angles) else float(theta0)


def oracle_tracked(p, x, angles, track, theta0):
    """p: params dict; x [M, F*hop] float32; track [F] indices into `angles`; theta0: the handle's theta.
    -> (y [F*hop] float32, Y [F, N] complex128)."""
    import oracle
    node = oracle.OracleNode(dict(p, theta=float(theta0)))
    H = p["hop"]
    F = x.shape[1] // H
    assert len(track) == F
    cur = float(theta0)
    ys, Ys = [], []
    for t in range(F):
        ang = angle_in_force(angles, track[t], theta0)
        if ang != cur:
            node.set_theta(ang)
            cur = ang
        y, Y = node.process_hop(x[:, t * H:(t + 1) * H], want_spectrum=True)
        ys.append(y.copy())
        Ys.append(Y.copy())
    return np.concatenate(ys), np.stack(Ys)


def from_peaks(peaks, maps, W, latency, min_peak, carry):
    """peaks [S, nb] int, maps [S, nb, A] float64 or None (every block publishes), carry [S] (or a scalar).
    Block b publishes peaks[s, b] when maps[s, b, peak] is not below min_peak (a peak outside the map is not looked up and does not
    publish).  Every frame of block b gets the index published by the latest block b' <= b - latency that published, carry[s] if there
    is none; carry_out[s] is what a block nb would get.  -> (track [S, nb * W] int32, carry_out [S] int32)."""
    peaks = np.asarray(peaks)
    S, nb = peaks.shape
    carry = np.broadcast_to(np.asarray(carry, np.int32), (S,)).copy()
    track = np.empty((S, nb * W), np.int32)
    out = carry.copy()

    def published(s, b):
        if maps is None:
            return True
        p = int(peaks[s, b])
        return 0 <= p < maps.shape[-1] and not (maps[s, b, p] < min_peak)

    def in_force(s, k):  # the latest publication of a block <= k
        for b in range(min(k, nb - 1), -1, -1):
            if published(s, b):
                return int(peaks[s, b])
        return int(carry[s])

    for s in range(S):
        for b in range(nb):
            track[s, b * W:(b + 1) * W] = in_force(s, b - latency)
        out[s] = in_force(s, nb - latency)
    return track, out
