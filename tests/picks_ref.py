"""Restatements for the multi-source pick tests (bf_doa_pick_device, bf_ctrack_from_picks_device; include/bfcore.h), in numpy and
written from the header's text, not from the kernels.  Test infrastructure only.

sep / pick: the picker of one map row.  from_picks: the column-track builder.  rows / grids: the row kinds and the candidate grids the
CPU and the GPU tests share."""
import numpy as np


def sep(a, b):
    """The header's steps, one at a time (numpy's fmod is C's): t = (a - b) + 180; r = fmod(t, 360); r < 0: r += 360; |r - 180|."""
    t = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) + 180.0
    r = np.fmod(t, 360.0)
    r = np.where(r < 0, r + 360.0, r)
    return np.abs(r - 180.0)


def pick(row, angles, k, min_sep_deg, rel_floor):
    """-> [k] int32: the picks of one row, strongest first, -1 in the unused places."""
    row, ang = np.asarray(row, np.float64), np.asarray(angles, np.float64)
    out = np.full(k, -1, np.int32)
    floor = rel_floor * row.max()
    free = np.ones(row.size, bool)
    for j in range(k):
        idx = np.flatnonzero(free)
        if idx.size == 0:
            break
        d = int(idx[np.argmax(row[idx])])  # the free index with the largest value; argmax keeps the first, so the lowest index on ties
        if row[d] < floor:
            break
        out[j] = d
        free[d] = False
        free[sep(ang, ang[d]) < min_sep_deg] = False
    return out


def pick_all(maps, angles, k, min_sep_deg, rel_floor):
    """maps [..., A] -> picks [..., k]"""
    maps = np.asarray(maps, np.float64)
    flat = maps.reshape(-1, maps.shape[-1])
    return np.stack([pick(r, angles, k, min_sep_deg, rel_floor) for r in flat]).reshape(maps.shape[:-1] + (k,))


def from_picks(picks, maps, n_angles, W, latency, min_peak, n_cols, carry):
    """picks [S, nb, k] int, maps [S, nb, A] float64 or None, carry [S, n_cols] (or a scalar).
    Block b publishes when picks[s, b, 0] is in 0 .. n_angles-1 and (without a map, or) the map value there is not below min_peak.  A
    publishing block updates column c < min(n_cols, k) when picks[s, b, c] is in 0 .. n_angles-1.  Every frame of block b gets, per
    column, the latest update by a block b' <= b - latency, carry[s, c] if there is none; carry_out is what a block nb would get.
    -> (track [S, nb * W, n_cols] int32, carry_out [S, n_cols] int32)."""
    picks = np.asarray(picks)
    S, nb, k = picks.shape
    carry = np.broadcast_to(np.asarray(carry, np.int32), (S, n_cols)).copy()
    track = np.empty((S, nb * W, n_cols), np.int32)
    out = carry.copy()

    def valid(p):
        return 0 <= int(p) < n_angles

    def publishes(s, b):
        p0 = picks[s, b, 0]
        return valid(p0) and (maps is None or not (maps[s, b, int(p0)] < min_peak))

    def in_force(v, kk):  # v[j]: the columns once blocks 0 .. j-1 have had their say
        return v[0] if kk < 0 else v[min(kk, nb - 1) + 1]

    for s in range(S):
        v = np.empty((nb + 1, n_cols), np.int32)
        v[0] = carry[s]
        for b in range(nb):
            v[b + 1] = v[b]
            if publishes(s, b):
                for c in range(min(n_cols, k)):
                    if valid(picks[s, b, c]):
                        v[b + 1, c] = picks[s, b, c]
        for b in range(nb):
            track[s, b * W:(b + 1) * W] = in_force(v, b - latency)
        out[s] = in_force(v, nb - latency)
    return track, out


# ---- shared cases --------------------------------------------------------------------------------------------------------------------
def grids(A, seed=0):
    """name -> [A] candidate angles: sorted with -180 and +180 both present, unsorted, beyond +-360, with duplicates."""
    rng = np.random.default_rng(1000 + 7 * A + seed)
    g = {"sorted": np.linspace(-180.0, 180.0, A) if A > 1 else np.array([20.0])}
    g["unsorted"] = rng.permutation(g["sorted"])
    g["wide"] = np.round(rng.uniform(-800.0, 800.0, A), 1)
    g["dup"] = np.round(rng.uniform(-180.0, 180.0, A) / 15.0) * 15.0
    return g


def rows(nr, A, seed=0):
    """[nr, A] map rows in [0, 1]: random, quantised to quarters (ties), constant, all zero, in turn."""
    rng = np.random.default_rng(2000 + 13 * A + seed)
    m = rng.random((nr, A))
    for r in range(nr):
        kind = r % 4
        if kind == 1:
            m[r] = np.round(m[r] * 4.0) / 4.0
        elif kind == 2:
            m[r] = 0.375
        elif kind == 3 and r % 8 == 7:
            m[r] = 0.0
    return m


PARAMS = [(k, ms, rf) for k in (1, 3, 16) for ms in (0.0, 10.0, 400.0) for rf in (0.0, 0.5, 1.0)]
