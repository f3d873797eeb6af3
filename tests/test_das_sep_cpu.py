"""The frame-pair kernels' delay-structured gains on the CPU (geometry.hpp das_sep_gains_w64_f64; tests/host_emul_sep restates the
kernel's new accumulation beside the per-bin table form): the host's separability check, the exception rows, the refusal of a table that
is not a delay, and the figure the GPU test hangs on."""
import numpy as np
import pytest

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene
from das_sep_util import GEOMETRIES, SEP_VS_TABLE_BOUND, load_sep_lib, sep_check, sep_das

PATH_CHAIN, PATH_FRAME_PAIR = 0, 1   # das_f64_plan.hpp DasF64Path


@pytest.fixture(scope="module")
def sep_lib():
    return load_sep_lib()


def _params(geo, theta, M=8):
    mics = GEOMETRIES[geo]
    M = M if mics is None else len(mics)
    return make_params("das", n_mics=M, theta=theta, **({} if mics is None else {"mics": mics}))


CASES = [("aira16-first-8 (1 = 7)", M, th) for M, th in ((2, -50.0), (3, -50.0), (5, -50.0), (8, -50.0), (8, 20.0), (8, -15.0), (8, 35.0), (8, 179.0))] + \
        [("all distinct", 8, 35.0), ("all distinct", 8, -70.0), ("2 = 3 and 5 = 6", 8, 35.0), ("symmetric about theta = 0", 6, 0.0)]


@pytest.mark.parametrize("geo,M,theta", CASES)
def test_separable_tables_reproduce_the_per_bin_table(sep_lib, geo, M, theta):
    """G[k3][k1] B[k2] -- the exception rows' entry times B in registers 13 and 2 -- against every entry of das_mic_gains_w64_f64 within the
    host's own bound: 2, 3, 5 and 8 microphones, the benchmark's geometry (the default, theta = 20 and -15 among the angles), no
    coinciding microphones, a look angle along a symmetry axis.  Bins 512 and 513 (register 2, B[0] = 1) are the table's bits; bin 511's
    entry (register 13) times B[15] is the table's value to the rounding of the entry itself."""
    c = sep_check(sep_lib, _params(geo, theta, M), theta)
    print(c)
    assert c["ok"] and c["path"] == PATH_FRAME_PAIR
    assert 0.0 <= c["worst"] <= c["bound"] < 1e-12      # the bound is (16 + 12 x the largest phase) x 2^-53: a few ulp per radian
    assert c["e512"] and c["e513"]
    assert c["d511"] <= 2.0 ** -52                        # one rounding of an entry of magnitude <= 1 / (M N), relative to 1 / (M N)
    # ... and with the factor the kernel really multiplies by, the slot's rounded tw2' B[15] (shared tw2' divided out): two more roundings
    assert c["d511_kernel"] <= 3 * 2.0 ** -52


@pytest.mark.parametrize("perturb", [(100, 3, 1e-12), (16, 1, 1e-12), (700, 5, 1e-11), (256, 7, 1e-10), (3, 2, -1e-12)])
def test_a_table_with_one_perturbed_entry_is_refused(sep_lib, perturb):
    """One weight off the delay by 1e-12 .. 1e-10 (a seed of the factors or any other bin): the check fails, `tables` is false and the
    decision is the chain."""
    p = _params("aira16-first-8 (1 = 7)", 20.0)
    assert sep_check(sep_lib, p, 20.0)["path"] == PATH_FRAME_PAIR
    c = sep_check(sep_lib, p, 20.0, perturb)
    print(c)
    assert not c["ok"] and c["worst"] > c["bound"] and c["path"] == PATH_CHAIN


def test_a_perturbed_quirk_bin_stays_what_the_table_says(sep_lib):
    """Bins 511 .. 513 are not on the ramp to begin with: their registers read the table's own entries, so whatever stands there is
    reproduced and the table is accepted."""
    c = sep_check(sep_lib, _params("aira16-first-8 (1 = 7)", 20.0), 20.0, (511, 2, 1e-6))
    assert c["ok"] and c["e512"] and c["e513"] and c["d511"] <= 2.0 ** -52


@pytest.mark.parametrize("geo,M,theta", [c for c in CASES if c[1] >= 5])
def test_new_form_against_table_form(sep_lib, geo, M, theta):
    """The backward transform's output in double, new form against table form, per output frame pair and relative to the pair's largest
    magnitude: within SEP_VS_TABLE_BOUND (the figure in EXPERIMENTS.md; the GPU test allows the kernel 4 x this against the new form).
    The summed spectrum per bin, relative to the spectrum's largest magnitude: within 4 x that."""
    p = _params(geo, theta, M)
    x = make_scene(p["n_mics"], 12, seed=3300 + p["n_mics"], mics=p["mics"])
    y0, u0, U0 = sep_das(sep_lib, p, theta, x, 0, True, True)
    y1, u1, U1 = sep_das(sep_lib, p, theta, x, 1, True, True)
    du = float((np.abs(u1 - u0).max(axis=1) / np.abs(u0).max(axis=1)).max())
    dU = float((np.abs(U1 - U0) / np.abs(U0).max(axis=1, keepdims=True)).max())
    print(f"per output frame pair {du:.3e}, per bin {dU:.3e}, float samples that differ {int((y0 != y1).sum())} of {y0.size}")
    assert du <= SEP_VS_TABLE_BOUND and dU <= 4 * SEP_VS_TABLE_BOUND
    assert int((y0 != y1).sum()) <= 2 and np.abs(y0 - y1).max() <= 2.0 ** -22 * np.abs(y0).max()


def test_new_form_against_the_oracle_hop_by_hop(sep_lib):
    """A few hundred frames of make_scene in float, hop by hop against the oracle: the new form differs in no more samples than a handful
    per 10^5 hops would give (measured: 0 of 153 600 for either form)."""
    import oracle
    F = 300
    p = _params("aira16-first-8 (1 = 7)", 20.0)
    x = make_scene(8, F, seed=42)
    y_ref = oracle.OracleNode(p).process(x)[0].astype(np.float32)
    n = [int((sep_das(sep_lib, p, 20.0, x, form)[0] != y_ref).sum()) for form in (0, 1)]
    print("float samples that differ from the oracle: table form %d, new form %d of %d" % (n[0], n[1], y_ref.size))
    assert n[0] <= 1 and n[1] <= 1
