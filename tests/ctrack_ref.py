"""Restatement for the column-track tests (bf_ctrack_*, include/bfcore.h).  Test infrastructure only.

oracle_ctracked: the reference mvdr / lcmv node with /theta and interferer messages landing between callbacks -- the oracle driven hop by
hop, set_theta called in front of hop t whenever column 0's angle in force changes and set_interference(c, angle, threshold=0.0) whenever
column c's does (a threshold of 0 never merges two interferers: the proximity rule is not part of a column track)."""
import numpy as np


def angle_in_force(angles, idx, own):
    """The index rule, per column: 0 .. len(angles)-1 names a candidate angle, anything else the column's own angle."""
    i = int(idx)
    return float(angles[i]) if 0 <= i < len(angles) else float(own)


def angles_in_force(angles, track, own):
    """track [F, n_cols] -> [F, len(own)] angles: columns the track does not carry stay at their own angle."""
    track = np.asarray(track)
    F, n_cols = track.shape
    assert 1 <= n_cols <= len(own)
    out = np.tile(np.asarray(own, np.float64), (F, 1))
    for t in range(F):
        for c in range(n_cols):
            out[t, c] = angle_in_force(angles, track[t, c], own[c])
    return out


def oracle_ctracked(p, x, angles, track, theta0, prepare=None, node=None):
    """p: params dict (mvdr or lcmv); x [M, F*hop] float32; track [F, n_cols] indices into `angles`, column 0 the look direction and
    column c interferer c; theta0: the handle's theta.  An out-of-range index means the create-time angle of that column (p["interf"]).
    prepare(node) (optional) runs once after the node exists and returns the columns' own angles from then on, look direction first
    -- for a structural interferer change in front of the batch.  node (optional): continue with this oracle node instead of a new one;
    the node is returned for the next call.
    -> (y [F*hop] float32, Y [F, N] complex128, node)."""
    import oracle
    track = np.asarray(track)
    if track.ndim == 1:
        track = track[:, None]
    if node is None:
        node = oracle.OracleNode(dict(p, theta=float(theta0)))
        node._ctrack_cur = [float(theta0)] + [float(a) for a in (p["interf"] if p["algo"] == "lcmv" else ())]
        node._ctrack_own = list(node._ctrack_cur)
    if prepare is not None:
        node._ctrack_own = [float(a) for a in prepare(node)]
        node._ctrack_cur = list(node._ctrack_own)
    own, cur = node._ctrack_own, node._ctrack_cur
    H = p["hop"]
    F = x.shape[1] // H
    assert track.shape[0] == F and 1 <= track.shape[1] <= len(own)
    want = angles_in_force(angles, track, own)
    ys, Ys = [], []
    for t in range(F):
        for c in range(len(own)):
            if want[t, c] != cur[c]:
                if c == 0:
                    node.set_theta(want[t, c])
                else:
                    k = node.set_interference(c, want[t, c], threshold=0.0)
                    assert k == len(own) - 1, "a column track never changes the interferer count"
                cur[c] = want[t, c]
        y, Y = node.process_hop(x[:, t * H:(t + 1) * H], want_spectrum=True)
        ys.append(y.copy())
        Ys.append(Y.copy())
    return np.concatenate(ys), np.stack(Ys), node
