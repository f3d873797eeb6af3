"""Inputs and measures of the dynamics tests (tests/test_dynamics_cpu.py, tests/test_dynamics_gpu.py): scenes with a stretch of exact
zeros, a faint stretch or one non-finite sample, and the per-hop comparison the contracts below are stated in.

Why per hop: several kernels take two signals through ONE complex transform (frames t and t + 1 of a microphone, 1024 / N frames of a
short period, two microphones, two output frames).  A transform's rounding error is 1e-16 (fp32: 1e-7) of the LOUDER signal and lands in
both, and so does a NaN.  A relative L2 over a whole signal cannot see an error that is large only against a quiet hop.

The strict contract (the library default: das in double and every fp64 node), `check_strict`:
  1. no sample is non-zero where the oracle is exactly zero;
  2. every other finite hop is within TOL_TIME of the oracle on its own norm;
  3. the set of non-finite output hops equals the oracle's.
The grouped contract (the BF_DAS_FUSED_F32 opt-in), `check_grouped`: G frames may share a transform (1024 / N below 512, else 2), so
  - |y - ref| <= TOL_TIME x max |ref| over the hops within G + 1 hops on either side (the project's bar at the scale of the loudest
    frame that can share the transform: frame t covers hops t - 1 and t, a group reaches G - 1 frames further);
  - exact zeros wherever the oracle has them and every input hop within G + 1 hops is zero;
  - the non-finite hops contain the oracle's and lie within that set widened by G hops each way.
"""
import functools

import numpy as np

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene

TOL_TIME = 1e-5      # the project's bar (tests/test_das_gpu.py), here applied per hop
SCALES = {"zero": 0.0, "m20": 2.0 ** -20, "m60": 2.0 ** -60}
F = 24               # frames of a case at hop 512


def stretch_scene(M, F, hop, seed, z0, z1, scale, mics=None):
    """make_scene(..., silent_frac=0.0) with input hops [z0, z1) multiplied by np.float32(scale)."""
    x = make_scene(M, F, hop=hop, seed=seed, mics=mics, silent_frac=0.0)
    x[:, z0 * hop:z1 * hop] *= np.float32(scale)
    return x


def nan_scene(M, F, hop, seed, h, mic, value=np.nan, sample=None, mics=None):
    """make_scene(..., silent_frac=0.0) with one sample of hop h of one microphone replaced by `value` (NaN or +Inf)."""
    x = make_scene(M, F, hop=hop, seed=seed, mics=mics, silent_frac=0.0)
    x[mic, h * hop + (hop // 3 if sample is None else sample)] = np.float32(value)
    return x


def dead_scene(M, F, hop, seed, mic, mics=None):
    """make_scene(..., silent_frac=0.0) with one microphone all zeros."""
    x = make_scene(M, F, hop=hop, seed=seed, mics=mics, silent_frac=0.0)
    x[mic] = 0.0
    return x


def hops_of(y, hop):
    y = np.asarray(y)
    return y.reshape(-1, hop)


def nonfinite_hops(y, hop):
    return {int(h) for h in np.flatnonzero(~np.isfinite(hops_of(y, hop)).all(axis=1))}


def zero_hops(y, hop):
    return {int(h) for h in np.flatnonzero(~hops_of(y, hop).any(axis=1))}


def per_hop(y, y_ref, hop):
    """({output hop: ||y_h - ref_h|| / ||ref_h||} over the hops where ref_h is finite and not all zero, the count of samples with
    ref == 0 and y != 0).  A non-finite y_h beside a finite ref_h counts as inf.  -0.0 == 0 passes."""
    a, b = hops_of(y, hop).astype(np.float64), hops_of(y_ref, hop).astype(np.float64)
    assert a.shape == b.shape
    rel = {}
    for h in range(b.shape[0]):
        if not np.isfinite(b[h]).all() or not b[h].any():
            continue
        if not np.isfinite(a[h]).all():
            rel[h] = float("inf")
            continue
        s = np.abs(b[h]).max()
        rel[h] = float(np.linalg.norm((a[h] - b[h]) / s) / np.linalg.norm(b[h] / s))
    with np.errstate(invalid="ignore"):
        stray = int(np.count_nonzero((b == 0) & (a != 0)))   # (NaN != 0 is True: a NaN over an oracle zero counts)
    return rel, stray


def check_strict(y, y_ref, hop, what="", unpinned=(), unpinned_abs=None):
    """`unpinned`: hops where the reference's own value is not pinned (say why at the call): left out of rules 1 and 2; with
    `unpinned_abs` they must instead agree within that fraction of the reference's largest finite magnitude."""
    unpinned = set(unpinned)
    rel, _ = per_hop(y, y_ref, hop)
    rel = {h: v for h, v in rel.items() if h not in unpinned}
    a, b = hops_of(y, hop), hops_of(y_ref, hop)
    keep = np.array([h not in unpinned for h in range(b.shape[0])])
    with np.errstate(invalid="ignore"):
        stray = int(np.count_nonzero((b[keep] == 0) & (a[keep] != 0)))
    worst = max(rel.items(), key=lambda kv: kv[1]) if rel else (None, 0.0)
    print(f"{what}: stray non-zeros {stray}, worst hop {worst[0]} rel {worst[1]:.3e}, non-finite hops {sorted(nonfinite_hops(y, hop))}")
    assert stray == 0, f"{what}: {stray} samples are non-zero where the oracle is exactly zero"
    assert worst[1] < TOL_TIME, f"{what}: hop {worst[0]} is {worst[1]:.3e} away from the oracle on its own norm"
    assert nonfinite_hops(y, hop) == nonfinite_hops(y_ref, hop), f"{what}: non-finite hops {sorted(nonfinite_hops(y, hop))}, oracle {sorted(nonfinite_hops(y_ref, hop))}"
    if unpinned_abs is not None:
        scale = np.abs(b[np.isfinite(b)]).max()
        for h in sorted(unpinned):
            if np.isfinite(b[h]).all():
                err = np.abs(a[h].astype(np.float64) - b[h]).max()
                assert err <= unpinned_abs * scale, f"{what}: unpinned hop {h}: |y - ref| = {err:.3e} against a scale of {scale:.3e}"


def identity_noise_hops(x, hop):
    """One microphone: das is the identity delayed by a hop (sqrt-Hann WOLA), output hop h = input hop h - 1.  Frames h - 1 and h make it
    and span input hops h - 2 .. h; their transforms leave 1e-16 of the loudest of those hops everywhere.  Where input hop h - 1 is more
    than 2^30 below that (hop 0: the zeros in front of the stream) the reference's output hop is its own FFT's rounding noise --
    oracle/np_oracle.py differs from the oracle by 1.3 on such a hop's own norm, and in which samples happen to be exact zeros."""
    mx = np.abs(np.nan_to_num(np.asarray(x, np.float64), nan=np.inf)).reshape(x.shape[0], -1, hop).max(axis=(0, 2))
    mx = np.concatenate([[0.0, 0.0], mx])   # mx[h + 2] = input hop h; hops -2, -1 are zeros
    return [h for h in range(len(mx) - 2) if mx[h + 1] < 2.0 ** -30 * max(mx[h], mx[h + 1], mx[h + 2])]


def group_frames(hop):
    """How many frames may share a transform in the fp32 opt-in: 1024 / N below period 512, else 2."""
    return 1024 // (2 * hop) if hop < 512 else 2


def check_grouped(y, y_ref, x, hop, what=""):
    """The fp32 opt-in's contract (module docstring).  x [M, F * hop]: the input, for the zero rule."""
    G = group_frames(hop)
    a, b = hops_of(y, hop).astype(np.float64), hops_of(y_ref, hop).astype(np.float64)
    nF = b.shape[0]
    in_zero = ~np.asarray(x).reshape(x.shape[0], nF, hop).any(axis=(0, 2))
    bad_ref = nonfinite_hops(y_ref, hop)
    bad = nonfinite_hops(y, hop)
    widened = {h + d for h in bad_ref for d in range(-G, G + 1) if 0 <= h + d < nF}
    assert bad_ref <= bad <= widened, f"{what}: non-finite hops {sorted(bad)}, oracle {sorted(bad_ref)}, G = {G}"
    fin = np.where(np.isfinite(b), np.abs(b), 0.0).max(axis=1)
    worst = 0.0
    for h in range(nF):
        if h in widened:
            continue
        lo, hi = max(0, h - G - 1), min(nF, h + G + 2)
        scale = fin[lo:hi].max()
        err = np.abs(a[h] - b[h]).max()
        if in_zero[lo:hi].all() and not b[h].any():
            assert not a[h].any(), f"{what}: hop {h} is not exactly zero although every input hop within {G + 1} is"
        worst = max(worst, err / scale if scale > 0 else (0.0 if err == 0 else float("inf")))
        assert err <= TOL_TIME * scale, f"{what}: hop {h}: |y - ref| = {err:.3e} against {scale:.3e} nearby"
    print(f"{what}: G = {G}, worst |y - ref| / nearby max = {worst:.3e}")


# ---- the matrix ----------------------------------------------------------------------------------------------------------------
# name -> builder arguments.  Stretches are 6 hops long, once from an even and once from an odd hop (both pairings of the transition);
# a non-finite sample sits in an even and an odd hop and in hops 0 and F - 1.  `k`: positions are in units of k hops (periods below 512
# scale them so that a stretch still spans 6 k >= 6 hops and a group of 1024 / N frames lies inside it).
def matrix(mic=3):
    m = {}
    for sc in SCALES:
        m[f"{sc}_even"] = dict(kind="stretch", z0=6, z1=12, scale=SCALES[sc])
        m[f"{sc}_odd"] = dict(kind="stretch", z0=7, z1=13, scale=SCALES[sc])
    for h in (0, 8, 9):
        m[f"nan_h{h}"] = dict(kind="nan", h=h, mic=mic, value=np.nan)
    m["nan_last"] = dict(kind="nan", h=-1, mic=mic, value=np.nan)   # hop F - 1
    m["inf_h8"] = dict(kind="nan", h=8, mic=mic, value=np.inf)
    m["inf_h9"] = dict(kind="nan", h=9, mic=mic, value=np.inf)
    m["nan_h9_mic0"] = dict(kind="nan", h=9, mic=0, value=np.nan)   # microphone 0 never enters a transform of the frame-pair kernels
    return m


MATRIX = matrix()
SEED = 777


def _pos(h, k):
    """Hop h of the hop-512 matrix at a period whose positions are in units of k hops: h k, plus one where h is odd (k even would lose it)."""
    return h * k + (1 if k > 1 and h % 2 else 0)


@functools.lru_cache(maxsize=None)
def scene(name, M=8, F=F, hop=512, seed=SEED, k=1):
    """The input of a case; shared, do not modify."""
    c = matrix(mic=min(3, M - 1))[name]
    if c["kind"] == "stretch":
        z0 = _pos(c["z0"], k)
        x = stretch_scene(M, F, hop, seed, z0, z0 + (c["z1"] - c["z0"]) * k, c["scale"])
    else:
        x = nan_scene(M, F, hop, seed, nan_hop(name, F, k), c["mic"], c["value"])
    x.setflags(write=False)
    return x


def nan_hop(name, F=F, k=1):
    """The input hop that holds the non-finite sample of a `nan` / `inf` case."""
    h = matrix()[name]["h"]
    return F - 1 if h < 0 else _pos(h, k)


def params(algo, M, hop=512, theta=20.0, **kw):
    return make_params(algo, n_mics=M, hop=hop, theta=theta, **kw)


@functools.lru_cache(maxsize=None)
def ref(algo, name, M=8, F=F, hop=512, seed=SEED, k=1, interf=(), want_spectrum=False):
    """The oracle's (y, Y) of a case; shared, do not modify."""
    import oracle
    y, Y = oracle.OracleNode(params(algo, M, hop, interf=interf)).process(scene(name, M, F, hop, seed, k), want_spectrum=want_spectrum)
    y.setflags(write=False)
    return y, Y


def zero_frame_hops(name):
    """The output hops of a `zero` case that hold a half of an all-zero frame: frames z0 + 1 .. z1 - 1, so hops z0 + 1 .. z1."""
    c = MATRIX[name]
    return range(c["z0"] + 1, c["z1"] + 1) if c["kind"] == "stretch" and c["scale"] == 0.0 else range(0)


def expected_nan_hops(h, F):
    """A non-finite sample in input hop h is in frames h and h + 1, whose halves make output hops h, h + 1, h + 2."""
    return {h, h + 1, h + 2} & set(range(F))
