"""A restatement of bf_ctrack_assign_device (include/bfcore.h) in numpy, written from the header's text, not from the kernel, from
beamform_amd/csrc/doa_assign.hpp or from controllers.assign_sources, and the case generators the CPU and the GPU tests share.  Test
infrastructure only.

assign: the contract's steps 1 to 7, one slot record per column.  cases / case_input: parameter sets and inputs.  scene_*: the
five-segment conversation of the scene tests."""
import numpy as np

import picks_ref

CAP = 2 ** 30


class _Slot:
    def __init__(self, rec):
        self.idx, self.hits, self.misses, self.out = (int(v) for v in rec)


def assign(picks, maps, angles, W, latency, min_peak, gate_deg, min_hits, max_coast, n_cols, state):
    """picks [S, nb, k] int, maps [S, nb, A] float64 or None, angles [A], state [S, n_cols, 4] int32 (or a scalar to fill it with).
    -> (track [S, nb * W, n_cols] int32, active [S, nb, n_cols] int32, state_out [S, n_cols, 4] int32)."""
    picks = np.asarray(picks)
    S, nb, k = picks.shape
    ang = np.asarray(angles, np.float64)
    A = ang.size
    state = np.broadcast_to(np.asarray(state, np.int32), (S, n_cols, 4)).copy()
    track = np.full((S, nb * W, n_cols), -99, np.int32)
    active = np.full((S, nb, n_cols), -99, np.int32)

    def is_index(v):
        return 0 <= v <= A - 1

    for s in range(S):
        slots = [_Slot(state[s, c]) for c in range(n_cols)]
        out_after = {-1: [sl.out for sl in slots]}  # block -> out as it stood after it; -1: on entry
        for b in range(nb):
            # 1. candidates
            p0 = int(picks[s, b, 0])
            publishes = is_index(p0) and (maps is None or not (maps[s, b, p0] < min_peak))
            cands = [int(picks[s, b, j]) for j in range(k) if is_index(int(picks[s, b, j]))] if publishes else []
            # 2. match
            live = [c for c in range(n_cols) if is_index(slots[c].idx)]
            dist = {(c, j): float(picks_ref.sep(ang[slots[c].idx], ang[cands[j]])) for c in live for j in range(len(cands))}
            slot_done, cand_done = set(), set()
            while True:
                pairs = [(d, c, j) for (c, j), d in dist.items() if c not in slot_done and j not in cand_done and d <= gate_deg]
                if not pairs:
                    break
                d, c, j = min(pairs)  # the smallest d; ties to the lowest c, then the lowest j
                # 3. a matched slot
                slots[c].idx = cands[j]
                slots[c].hits = min(slots[c].hits + 1, CAP)
                slots[c].misses = 0
                slot_done.add(c)
                cand_done.add(j)
            # 4. an unmatched live slot
            for c in live:
                if c in slot_done:
                    continue
                if slots[c].hits < min_hits:
                    slots[c].idx = -1
                else:
                    slots[c].misses = min(slots[c].misses + 1, CAP)
                    if slots[c].misses > max_coast:
                        slots[c].idx = -1
            # 5. births
            born = set()
            for j in range(len(cands)):
                if j in cand_done:
                    continue
                free = [c for c in range(n_cols) if not is_index(slots[c].idx)]
                if free:
                    sl = slots[free[0]]
                    sl.idx, sl.hits, sl.misses = cands[j], 1, 0
                    born.add(free[0])
            # 6. out and active
            for c, sl in enumerate(slots):
                if is_index(sl.idx) and sl.hits >= min_hits:
                    sl.out = sl.idx
                active[s, b, c] = 1 if (c in slot_done or c in born) and sl.hits >= min_hits else 0
            out_after[b] = [sl.out for sl in slots]
        # 7. frames
        for b in range(nb):
            track[s, b * W:(b + 1) * W] = out_after[b - latency if b - latency >= 0 else -1]
        for c, sl in enumerate(slots):
            state[s, c] = np.array([sl.idx, sl.hits, sl.misses, sl.out], np.int64).astype(np.int32)
    return track, active, state


# ---- shared cases --------------------------------------------------------------------------------------------------------------------
BAD_PICKS = (None, -7, 2 ** 31 - 1)  # None: n_angles itself


def pick_rows(S, nb, k, A, kind, seed):
    """[S, nb, k] int32 pick rows.  distinct: valid and (where A allows) distinct; holes: -1 in some places, the first included;
    bad: out-of-range values (n_angles, -7, 2^31 - 1) in some places; repeat: indices repeated inside a row; none: all -1."""
    rng = np.random.default_rng(5000 + 131 * S + 17 * nb + 7 * k + A + seed)
    if kind == "none":
        return np.full((S, nb, k), -1, np.int32)
    if kind == "repeat" or A < k:
        p = rng.integers(0, A, (S, nb, k))
        if kind == "repeat":
            p[..., 1:] = np.where(rng.random((S, nb, k - 1)) < 0.5, p[..., :1], p[..., 1:])
    else:
        p = np.stack([rng.permutation(A)[:k] for _ in range(S * nb)]).reshape(S, nb, k)
    p = p.astype(np.int64)
    if kind == "holes":
        p[rng.random(p.shape) < 0.3] = -1
    if kind == "bad":
        hit = rng.random(p.shape) < 0.3
        bad = np.array([A if v is None else v for v in BAD_PICKS], np.int64)
        p[hit] = bad[rng.integers(0, bad.size, int(hit.sum()))]
    return p.astype(np.int32)


KINDS = ("distinct", "holes", "bad", "repeat", "none")


def slow_rows(S, nb, k, A, seed):
    """Pick rows that hold talkers: per stream up to k indices that drift by a step per block, leave for a few blocks and come back,
    in a row order that changes from block to block -- so that columns are matched, coast, are freed and are born."""
    rng = np.random.default_rng(6000 + 131 * S + 17 * nb + 7 * k + A + seed)
    p = np.full((S, nb, k), -1, np.int32)
    for s in range(S):
        pos = rng.integers(0, A, k)
        for b in range(nb):
            pos = (pos + rng.integers(-1, 2, k)) % A
            on = rng.random(k) < 0.7
            row = [int(v) for v, o in zip(pos, on) if o]
            rng.shuffle(row)
            p[s, b, :len(row)] = row
    return p


def garbage_state(S, n_cols, A, seed):
    """[S, n_cols, 4] int32: live slots with sane counters, live slots with extreme counters, free slots with idx out of range (-1, A,
    -2^31, 2^31 - 1) and garbage hits / misses, any `out`."""
    rng = np.random.default_rng(7000 + 31 * S + n_cols + A + seed)
    st = np.empty((S, n_cols, 4), np.int64)
    st[..., 0] = rng.integers(0, A, (S, n_cols))
    st[..., 1] = rng.integers(0, 5, (S, n_cols))
    st[..., 2] = rng.integers(0, 5, (S, n_cols))
    st[..., 3] = rng.integers(-1, A, (S, n_cols))
    ext = np.array([2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, -2 ** 31, -1, 0], np.int64)
    big = rng.random((S, n_cols)) < 0.3
    st[..., 1][big] = ext[rng.integers(0, ext.size, int(big.sum()))]
    big = rng.random((S, n_cols)) < 0.3
    st[..., 2][big] = ext[rng.integers(0, ext.size, int(big.sum()))]
    free = rng.random((S, n_cols)) < 0.4
    off = np.array([-1, A, -2 ** 31, 2 ** 31 - 1, A + 5], np.int64)
    st[..., 0][free] = off[rng.integers(0, off.size, int(free.sum()))]
    far = rng.random((S, n_cols)) < 0.2
    st[..., 3][far] = off[rng.integers(0, off.size, int(far.sum()))]
    return st.astype(np.int32)


def maps_for(S, nb, A, seed):
    rng = np.random.default_rng(8000 + 31 * S + 17 * nb + A + seed)
    m = rng.random((S, nb, A))
    m[rng.random((S, nb)) < 0.1] = np.nan  # a NaN publishes
    return m


# the values the issue lists; the sweep below walks them so that every value of every parameter meets several values of the others
K_SET, C_SET, GATE_SET, HITS_SET, COAST_SET, LAT_SET, W_SET, NB_SET, A_SET = ((1, 3, 16), (1, 2, 16), (0.0, 10.0, 400.0), (1, 2, 3),
                                                                              (0, 2, 2 ** 30), (0, 1, 3), (1, 4), (1, 2, 67), (1, 5, 180))
GRID_NAMES = ("sorted", "unsorted", "wide", "dup")


def sweep():
    """-> a list of parameter dicts: for every (grid kind, A, row kind) a rotation through the value sets above, so that every value
    of every set and every pair of (k, n_cols) and (gate, min_hits, max_coast) turns up."""
    out, n = [], 0
    for A in A_SET:
        for name in GRID_NAMES:
            for kind in KINDS + ("slow",):
                for rep in range(3):
                    out.append(dict(A=A, grid=name, kind=kind, k=K_SET[n % 3], n_cols=C_SET[(n // 3) % 3], gate=GATE_SET[(n + rep) % 3],
                                    min_hits=HITS_SET[(n // 2) % 3], max_coast=COAST_SET[(n // 5) % 3], latency=LAT_SET[(n // 7) % 3],
                                    W=W_SET[n % 2], nb=NB_SET[(n // 4 + rep) % 3], with_map=bool((n // 3) % 2), seed=n))
                    n += 1
    return out


def case_input(c, S):
    """-> (picks [S, nb, k], maps [S, nb, A] or None, angles [A], min_peak, state [S, n_cols, 4]) of one sweep entry."""
    A, nb, k = c["A"], c["nb"], c["k"]
    angles = np.ascontiguousarray(picks_ref.grids(A)[c["grid"]], np.float64)
    picks = slow_rows(S, nb, k, A, c["seed"]) if c["kind"] == "slow" else pick_rows(S, nb, k, A, c["kind"], c["seed"])
    maps = maps_for(S, nb, A, c["seed"]) if c["with_map"] else None
    state = garbage_state(S, c["n_cols"], A, c["seed"]) if c["seed"] % 3 == 0 else np.full((S, c["n_cols"], 4), -1, np.int32)
    return picks, maps, angles, (0.5 if c["with_map"] else 0.0), state


def run(fn, c, picks, maps, angles, min_peak, state):
    return fn(picks, maps, angles, c["W"], c["latency"], min_peak, c["gate"], c["min_hits"], c["max_coast"], c["n_cols"], state)


# ---- the conversation of the scene tests ---------------------------------------------------------------------------------------------
SCENE_GRID = np.arange(-180.0, 180.0, 2.0)
SCENE_M, SCENE_W, SCENE_SEG_FRAMES = 8, 16, 32
SCENE_SEGMENTS = ((40, 20.0, (-60.0,), 0.2, 0.05), (41, -60.0, (20.0,), 0.2, 0.05), (42, -60.0, (), 0.2, None),
                  (43, 20.0, (-60.0,), 0.2, 0.05), (44, 110.0, (20.0,), 0.1, 0.2))
SCENE_PICK = (3, 15.0, 0.04)                      # k, min_sep_deg, rel_floor
SCENE_ASSIGN = dict(n_cols=3, gate=20.0, min_hits=2, max_coast=4, latency=1)
I20, IM60, I110 = 100, 60, 145                    # grid indices of 20, -60 and 110 degrees
SCENE_PICKS = [[I20, IM60]] * 2 + [[IM60, I20]] * 2 + [[IM60]] * 2 + [[I20, IM60]] * 2 + [[I20, I110]] * 2
SCENE_OUT = [[-1, -1, -1]] + [[I20, IM60, -1]] * 8 + [[I20, IM60, I110]]
SCENE_ACTIVE = [[0, 0, 0]] + [[1, 1, 0]] * 3 + [[0, 1, 0]] * 2 + [[1, 1, 0]] * 2 + [[1, 0, 0]] + [[1, 0, 1]]


def scene_audio():
    """[8, 160 * 512] float32: five segments of two blocks each -- 20 over -60, -60 over 20, -60 alone, 20 over -60, 110 over 20."""
    from beamform_amd.synth import make_scene
    segs = []
    for seed, theta, interf, sig_s, sig_i in SCENE_SEGMENTS:
        kw = dict(seed=seed, theta_s=theta, interferers=interf, sigma_s=sig_s, silent_frac=0.0)
        if sig_i is not None:
            kw["sigma_i"] = sig_i
        segs.append(make_scene(SCENE_M, SCENE_SEG_FRAMES, 512, 48000.0, **kw))
    return np.ascontiguousarray(np.concatenate(segs, axis=1), np.float32)


def outs_of(track, state, W, latency=1):
    """[nb, n_cols]: out after every block of one stream, read from a latency-1 track and the final state."""
    nb = track.shape[0] // W
    assert latency == 1
    return np.concatenate([track.reshape(nb, W, -1)[1:, 0], state[None, :, 3]])
