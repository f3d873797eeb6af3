"""What a batch launched is what its plan said: one warm-up batch, one batch under launch_trace, and the traced kernel list against
chain_decide (csrc/chain_plan.hpp, through tests/host_emul) formatted for the device's own CU count."""
import pytest
import torch

from beamform_amd.capi import BF_DAS_F64, BF_INTERLEAVED, BF_PLANAR, BF_PRECISION_MIXED, BF_PRECISION_REFERENCE, Beamformer, launch_trace
from beamform_amd.params import make_params
from chain_plan_util import chain_kernels, params_plan

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(emul_lib, algo, M=8, hop=512, F=5, streams=1, layout=BF_PLANAR, dump=False, mixed=False, interf=()):
    p = make_params(algo, n_mics=M, hop=hop, interf=interf)
    bf = Beamformer(p, layout=layout, das_impl=BF_DAS_F64, precision=BF_PRECISION_MIXED if mixed else BF_PRECISION_REFERENCE, n_streams=streams)
    shape = (streams, M, F * hop) if layout == BF_PLANAR else (streams, F * hop, M)
    x = torch.rand(shape, device="cuda") - 0.5
    y = torch.empty((streams, F * hop), device="cuda")
    spec = torch.empty((streams, F, 2 * hop, 2), device="cuda", dtype=torch.float64) if dump else None
    sp = spec.data_ptr() if dump else 0
    bf.process_device(x.data_ptr(), F, y.data_ptr(), sp)
    with launch_trace() as t:
        bf.process_device(x.data_ptr(), F, y.data_ptr(), sp)
    torch.cuda.synchronize()
    bf.close()
    d = params_plan(emul_lib, p, F, _cus(), layout=layout, streams=streams, dump=dump, mixed=mixed)
    assert [k.replace("bf::", "") for k in t.kernels] == chain_kernels(d, 2 * hop), (t.kernels, d)
    return d


@pytest.mark.parametrize("case", [
    dict(algo="mvdr", hop=64), dict(algo="mvdr", hop=512), dict(algo="mvdr", hop=1024), dict(algo="mvdr", hop=2048),
    dict(algo="mvdr", M=16), dict(algo="mvdr", mixed=True), dict(algo="lcmv", M=3, interf=(-60.0, 90.0)),
    dict(algo="phase", layout=BF_INTERLEAVED), dict(algo="phase", dump=True), dict(algo="das", M=16), dict(algo="gsc", M=3),
    dict(algo="mcra", M=1)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_launched_kernels_are_the_plan(emul_lib, case):
    """5 frames: an odd count leaves the frame-pair ISTFT a partial pair."""
    _check(emul_lib, **case)


@pytest.mark.parametrize("below", [0, 1])
def test_phasempf_recursion_threshold_follows_the_cu_count(emul_lib, below):
    """mpf_rec_istft_kernel from ceil(n_cus / 4) streams on; one stream fewer: mpf_recursion_kernel + the backward transform."""
    d = _check(emul_lib, "phasempf", F=2, streams=(_cus() + 3) // 4 - below)
    assert d["rec"] == (1 if below else 2)


@pytest.mark.parametrize("below", [0, 1])
def test_gss_lane_threshold_follows_the_cu_count(emul_lib, below):
    """gss_lane_kernel from two wavefronts per CU on (nine wavefronts per stream at N = 1024): ceil(2 n_cus / 9) streams."""
    d = _check(emul_lib, "gss", F=2, streams=(2 * _cus() + 8) // 9 - below, interf=(-60.0, 90.0))
    assert d["bins"] == (8 if below else 9)
