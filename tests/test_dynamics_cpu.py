"""The expectations of the dynamics tests, on the CPU (tests/dynamics_cases.py): the oracle alone satisfies the conditions the GPU tests
rest on, a second implementation (oracle/np_oracle.py) pins its values per hop, and the CPU restatements of the das kernels
(tests/host_emul) meet the strict contract on the same inputs -- the frame-pair kernel's because it carries the kernel's pairing rule."""
import ctypes as C

import numpy as np
import pytest

import dynamics_cases as dc

NAMES = list(dc.MATRIX)
STRETCH = [n for n in NAMES if dc.MATRIX[n]["kind"] == "stretch"]
NONFIN = [n for n in NAMES if dc.MATRIX[n]["kind"] == "nan"]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("name", [n for n in STRETCH if n.startswith("zero")])
@pytest.mark.parametrize("algo", ["das", "phase", "mvdr", "gss", "mcra"])
def test_oracle_zero_stretch_gives_exact_zero_hops(algo, name):
    """Input hops [z0, z1) zero: frames z0 + 1 .. z1 - 1 are zero, so output hops z0 + 2 .. z1 - 1 are (frame t lands in hops t, t + 1)."""
    c = dc.MATRIX[name]
    M = 4 if algo == "mvdr" else 8
    y, _ = dc.ref(algo, name, M=M, interf=(-60.0,) if algo == "gss" else ())
    want = set(range(c["z0"] + 2, c["z1"]))
    assert len(want) >= 4
    assert want <= dc.zero_hops(y, 512), (sorted(want), sorted(dc.zero_hops(y, 512)))
    if algo == "das":   # a linear node: nothing else is zero
        assert dc.zero_hops(y, 512) == want


@pytest.mark.parametrize("name", NONFIN)
@pytest.mark.parametrize("algo", ["das", "phase"])
def test_oracle_nonfinite_sample_reaches_three_hops(algo, name):
    y, _ = dc.ref(algo, name)
    assert dc.nonfinite_hops(y, 512) == dc.expected_nan_hops(dc.nan_hop(name), dc.F)


NOT_INF = [n for n in NAMES if not n.startswith("inf")]


@pytest.mark.parametrize("algo,M,interf,name", [("das", M, (), n) for M in (8, 3) for n in NAMES]
                         + [("mvdr", 4, (), n) for n in NOT_INF] + [("gss", 8, (-60.0,), n) for n in NOT_INF])
def test_second_implementation_agrees_per_hop(algo, M, interf, name):
    """oracle.OracleNode and oracle/np_oracle.py per hop within 1e-9: both end in float32 stores, so a hop of 512 samples differs by a
    handful of last-place flips at most.  +Inf goes through das only: in mvdr and gss the two disagree about which later hops are
    non-finite (the magnitude gates see inf - inf of two different FFT libraries), so the reference's own answer is not pinned there."""
    from oracle import np_oracle
    y, _ = dc.ref(algo, name, M=M, interf=interf)
    y2, _ = np_oracle.process(dc.params(algo, M, interf=interf), dc.scene(name, M))
    rel, stray = dc.per_hop(y2, y, 512)
    assert stray == 0
    assert dc.nonfinite_hops(y2, 512) == dc.nonfinite_hops(y, 512)
    assert max(rel.values()) < 1e-9, max(rel.items(), key=lambda kv: kv[1])


def _emul(emul_lib, which, M, hop, name, F=dc.F, k=1):
    p = dc.params("das", M, hop)
    x = dc.scene(name, M, F, hop, dc.SEED, k)
    y = np.full(F * hop, np.nan, np.float32)
    mx = np.array([m[0] for m in p["mics"]])
    my = np.array([m[1] for m in p["mics"]])
    sr, th = C.c_double(48000.0), C.c_double(p["theta"])
    if which == "pair_f64":
        emul_lib.emul_das_pair_f64(M, sr, _ptr(mx), _ptr(my), th, _ptr(x), C.c_long(F), _ptr(y))
    elif which == "fused":
        emul_lib.emul_das_fused(M, hop, sr, _ptr(mx), _ptr(my), th, _ptr(x), C.c_long(F), _ptr(y))
    elif which == "small_ruled":
        emul_lib.emul_das_small_ruled(M, hop, sr, _ptr(mx), _ptr(my), th, _ptr(x), C.c_long(F), _ptr(y))
    else:
        emul_lib.emul_das_small(M, hop, sr, _ptr(mx), _ptr(my), th, _ptr(x), C.c_long(F), _ptr(y))
    return y, dc.ref("das", name, M, F, hop, dc.SEED, k)[0], x


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("M", [8, 3])
def test_emulated_frame_pair_das_meets_the_strict_contract(emul_lib, M, name):
    """das_f64_pair_kernel's arithmetic with its pairing rule: frames t, t + 1 share a transform only if both are finite and the
    largest magnitudes of their three hops are within 2^4 of each other (das_f64_plan.hpp das_f64_may_pair)."""
    y, y_ref, _ = _emul(emul_lib, "pair_f64", M, 512, name)
    dc.check_strict(y, y_ref, 512, f"emul_das_pair_f64 M={M} {name}")


@pytest.mark.parametrize("name", NAMES)
def test_emulated_fused_das_meets_the_strict_contract(emul_lib, name):
    """das_fused_kernel at period 512 takes two MICROPHONES of one frame through a transform: frames never meet."""
    y, y_ref, _ = _emul(emul_lib, "fused", 8, 512, name)
    dc.check_strict(y, y_ref, 512, f"emul_das_fused {name}")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("hop,k", [(256, 2), (64, 8)])
def test_emulated_frame_interleaving_das_meets_the_strict_contract(emul_lib, hop, k, name):
    """1024 / N frames interleaved into one transform, with the frame-pair kernels' rule applied to the group (emul_das_small_ruled): a
    group shares its transforms only if every frame is finite and within the rule's span of the others.  What this guards: the strict
    contract is what the formulation is asked for, and as the kernel runs it (no rule: the test below) it cannot meet it -- zeros, 2^-60
    and NaN all fail.  The ruled variant shows that the rule, applied per group, is sufficient at periods 64 and 256, should the fp32
    opt-in ever be held to the strict contract; it covers no library code today."""
    y, y_ref, _ = _emul(emul_lib, "small_ruled", 8, hop, name, F=dc.F * k, k=k)
    dc.check_strict(y, y_ref, hop, f"emul_das_small_ruled hop={hop} {name}")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("hop,k", [(256, 2), (64, 8)])
def test_emulated_frame_interleaving_das_meets_the_grouped_contract(emul_lib, hop, k, name):
    """The formulation as das_fused_kernel's group mode runs it (emul_das_small, no rule) under the fp32 opt-in's contract."""
    y, y_ref, x = _emul(emul_lib, "small", 8, hop, name, F=dc.F * k, k=k)
    dc.check_grouped(y, y_ref, x, hop, f"emul_das_small hop={hop} {name}")


def test_per_hop_measure_sees_what_a_whole_signal_norm_cannot():
    """The measure itself: an error of 1e-16 of the loud part inside a stretch 2^-60 below it is invisible to a relative L2 over the
    signal and unmistakable per hop; -0.0 over an oracle zero is no stray sample, 1e-30 is."""
    ref = np.ones(4 * 512, np.float32)
    ref[512:1024] = np.float32(2.0 ** -60)
    ref[1024:1536] = 0.0
    y = ref.copy()
    y[512:1024] += np.float32(1e-16)
    y[1024] = -0.0
    rel, stray = dc.per_hop(y, ref, 512)
    assert set(rel) == {0, 1, 3} and stray == 0
    assert rel[1] > 10 and rel[0] == 0 and np.linalg.norm(y - ref) / np.linalg.norm(ref) < 1e-14
    y[1025] = 1e-30
    assert dc.per_hop(y, ref, 512)[1] == 1
    y[1536] = np.nan
    assert dc.per_hop(y, ref, 512)[0][3] == float("inf")


def _bits(v):
    return int(np.float32(v).view(np.uint32)) & 0x7FFFFFFF


def test_pairing_rule_itself(emul_lib):
    """das_f64_may_pair (das_f64_plan.hpp) on the bit patterns of three hop maxima: level audio pairs (or every test here would pass with
    every frame alone, three times slower), zeros pair with zeros only, a span of 2^4 in the exponents pairs and 2^5 does not, Inf and NaN
    never pair; and on the scene every case starts from, every pair of the stream is allowed to share its transforms."""
    may = lambda a, b, c: bool(emul_lib.emul_das_may_pair(_bits(a), _bits(b), _bits(c)))   # noqa: E731
    assert may(0.3, 0.5, 0.2) and may(0.0, 0.0, 0.0) and may(1.0, 16.0, 1.0) and may(1.9, 16.0, 31.9)
    assert not may(0.0, 0.5, 0.5) and not may(0.5, 0.5, 0.0) and not may(0.5, 0.0, 0.5)
    assert not may(1.0, 32.0, 1.0) and not may(32.0, 1.0, 1.0) and not may(1.0, 1.0, 2.0 ** -20)
    assert not may(np.inf, 1.0, 1.0) and not may(1.0, np.nan, 1.0) and not may(1.0, 1.0, np.inf)
    assert may(1e-40, 1e-39, 0.0)   # subnormals share the exponent of zero
    x = dc.stretch_scene(8, dc.F, 512, dc.SEED, 0, 0, 1.0)
    m = [0.0] + list(np.abs(x[1:]).reshape(7, dc.F, 512).max(axis=(0, 2)))   # hop -1 in front: the zeros before the stream
    assert not may(m[0], m[1], m[2])                                          # so the first pair goes alone ...
    assert all(may(m[t], m[t + 1], m[t + 2]) for t in range(2, dc.F, 2))      # ... and every other one shares


def test_forced_chunk_plan_puts_every_pair_at_a_chunk_boundary(emul_lib):
    """The premise of test_dynamics_gpu.test_pairs_done_again_at_chunk_boundaries: by default the 24 frames of a case are two chunks
    (frames 0 and 16), so a pair the pairing rule does again sits inside a chunk; BF_DAS_F64_SCHED=1,1 makes every pair a chunk of its own,
    first and last at once, its two outer halves completed by atomic adds."""
    def starts(env):
        cap = 64
        st, t0, n = (np.zeros(cap, np.int32), np.zeros(cap, np.int64), np.zeros(cap, np.int64))
        grid = C.c_int(0)
        k = emul_lib.emul_das_plan(C.c_long(dc.F), 1, 256, env, cap, _ptr(st), _ptr(t0), _ptr(n), C.byref(grid))
        return sorted(int(v) for v in t0[:k]), sorted(int(v) for v in n[:k])
    assert starts(None)[0] == [0, 16]
    assert starts(b"1,1") == (list(range(0, dc.F, 2)), [2] * (dc.F // 2))
